"""f2_score_track: the decisions of a strided evaluation reduced to the time columns of a picture, against a NumPy / math.fsum
referee of the header's definition - counts, minimum and maximum exact, the mean inside the bound of any summation order; NaN
scores, bit identity between calls and memory spaces, placement between guard bands, argument errors. Shapes are the smallest at
which each thing can go wrong (the conditions the cases must meet are asserted on the referee alone)."""
import math

import numpy as np
import pytest

from devmem import Arena
from f2cnn_amd import _lib
from f2cnn_amd.scripts.plotting import PlottingProcessing as pp

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 37, 5000, 20000)      # per utterance of every call
HOPS = (1, 7, 160)
ORIGIN = 800
WIDTHS = (1, 7, 64, 300)
INNER = ((790, 830), 64)            # m < width: neighbouring columns repeat a sample
CASES = [(hop, W, "whole") for hop in HOPS for W in WIDTHS] + [(hop, INNER[1], "inner") for hop in HOPS]
MEMS = (_lib.MEM_HOST, _lib.MEM_DEVICE)
WO = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int64)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def decisions():
    """scores (n, 2) = (1 - p, p), p uniform in [0, 1) as float32; random labels"""
    rng = np.random.default_rng(114)
    p = rng.random(int(WO[-1])).astype(np.float32)
    scores = np.ascontiguousarray(np.stack([np.float32(1) - p, p], axis=1))
    return scores, rng.integers(0, 2, int(WO[-1])).astype(np.uint8)


def spans_of(hop, kind):
    if kind == "inner":
        return np.array([INNER[0]] * len(ROWS), np.int64)
    return np.array([[0, 2 * ORIGIN + n * hop] for n in ROWS], np.int64)


def owned_rows(n, span, hop, W):
    """(j_lo, j_hi) per column: the rows j of an utterance of n rows with lo_x <= ORIGIN + j hop < hi_x"""
    s, e = int(span[0]), int(span[1])
    if e == s:
        return np.zeros(W, np.int64), np.zeros(W, np.int64)
    lo, hi = pp.column_edges(e - s, W, s)
    t = ORIGIN + hop * np.arange(n, dtype=np.int64)
    return np.searchsorted(t, lo, side="left"), np.searchsorted(t, hi, side="left")


_referee = {}


def referee(decisions, hop, W, kind):
    """(track (U, W, 5) with the fsum mean, exact) computed once per case"""
    key = (hop, W, kind)
    if key not in _referee:
        scores, labels = decisions
        spans = spans_of(hop, kind)
        out = np.full((len(ROWS), W, 5), np.nan)
        for u, n in enumerate(ROWS):
            p = scores[WO[u]:WO[u + 1], 1]
            lab = labels[WO[u]:WO[u + 1]]
            j0, j1 = owned_rows(n, spans[u], hop, W)
            for x in range(W):
                seg = p[j0[x]:j1[x]]
                out[u, x, 0], out[u, x, 1] = len(seg), np.count_nonzero(lab[j0[x]:j1[x]])
                if len(seg):
                    out[u, x, 2] = math.fsum(seg.astype(np.float64).tolist()) / len(seg)
                    out[u, x, 3], out[u, x, 4] = seg.min(), seg.max()
        _referee[key] = out
    return _referee[key]


def run(ctx, scores, labels, wo, spans, origin, hop, W, mem, fill=-7.0):
    U = len(wo) - 1
    track = np.full((U, W, 5), fill)
    if mem == _lib.MEM_HOST:
        ctx.score_track(scores, labels, wo, spans, origin, hop, W, track, mem)
        return track
    d_s, d_l, d_t = ctx.malloc(max(scores.nbytes, 8)), ctx.malloc(max(labels.nbytes, 8)), ctx.malloc(max(track.nbytes, 8))
    try:
        ctx.h2d(d_s, scores)
        ctx.h2d(d_l, labels)
        ctx.h2d(d_t, track)
        ctx.score_track(d_s, d_l, wo, spans, origin, hop, W, d_t, mem)
        ctx.synchronize()
        ctx.d2h(track, d_t)
    finally:
        for p in (d_s, d_l, d_t):
            ctx.free(p)
    return track


def test_cases_reach_every_path():
    """on the referee's row counts alone: the conditions the issue sets for the cases"""
    counts = {c: np.stack([np.subtract(*owned_rows(n, spans_of(c[0], c[2])[u], c[0], c[1])[::-1]) for u, n in enumerate(ROWS)])
              for c in CASES}
    last = len(ROWS) - 1
    assert any(k[last, 0] == 0 and k[last, -1] == 0 and k[last].max() > 0 for k in counts.values())      # empty at each end
    assert any((k == 1).any() for k in counts.values())
    assert any(((k > 64) & (k <= 4096)).any() for k in counts.values())
    assert any((k > 4096).any() for k in counts.values())
    for hop in HOPS:                                                                                       # two columns share a row
        j0, j1 = owned_rows(ROWS[last], INNER[0], hop, INNER[1])
        assert any(j1[x] > j0[x] and j0[x] == j0[x + 1] and j1[x] == j1[x + 1] for x in range(INNER[1] - 1))
        assert (j1 - j0).sum() > min(ROWS[last], -(-(INNER[0][1] - ORIGIN) // hop))


@pytest.mark.parametrize("hop,W,kind", CASES)
def test_track_against_the_definition(ctx, decisions, hop, W, kind):
    scores, labels = decisions
    want = referee(decisions, hop, W, kind)
    spans = spans_of(hop, kind)
    got = [run(ctx, scores, labels, WO, spans, ORIGIN, hop, W, mem) for mem in MEMS]
    again = run(ctx, scores, labels, WO, spans, ORIGIN, hop, W, _lib.MEM_DEVICE)
    assert got[0].tobytes() == got[1].tobytes() == again.tobytes()          # the same bits in both memory spaces and on every call
    t = got[0]
    for k in (0, 1, 3, 4):
        assert np.array_equal(t[..., k], want[..., k], equal_nan=True), k
    empty = want[..., 0] == 0
    assert np.isnan(t[..., 2][empty]).all() and not np.isnan(t[..., 2][~empty]).any()
    # any order of adding `rows` non-negative float64 terms, then one division: (rows + 2) * 2^-53 relative
    bound = (want[..., 0] + 2) * 2.0 ** -53 * want[..., 2]
    err = np.abs(t[..., 2] - want[..., 2])
    print(f"hop {hop} W {W} {kind}: worst mean error / bound {np.nanmax(np.where(empty, 0.0, err / np.maximum(bound, 1e-300))):.3f}")
    assert (err[~empty] <= bound[~empty]).all()


def test_one_nan_score_spoils_its_column_only(ctx, decisions):
    scores, labels = decisions
    hop, W = 7, 64
    want = referee(decisions, hop, W, "whole")
    u, j = 3, 1234
    j0, j1 = owned_rows(ROWS[u], spans_of(hop, "whole")[u], hop, W)
    x = int(np.flatnonzero((j0 <= j) & (j < j1))[0])
    bad = scores.copy()
    bad[WO[u] + j, 1] = np.nan
    clean = run(ctx, scores, labels, WO, spans_of(hop, "whole"), ORIGIN, hop, W, _lib.MEM_DEVICE)
    for mem in MEMS:
        t = run(ctx, bad, labels, WO, spans_of(hop, "whole"), ORIGIN, hop, W, mem)
        assert np.isnan(t[u, x, 2:]).all() and np.array_equal(t[u, x, :2], want[u, x, :2])
        t[u, x, 2:] = clean[u, x, 2:]
        assert t.tobytes() == clean.tobytes()


@pytest.mark.parametrize("mis", ((1, 3, 1), (3, 5, 7)))
def test_outputs_between_guard_bands_at_odd_alignments(ctx, decisions, mis):
    scores, labels = decisions
    hop, W = 7, 300
    with Arena(ctx) as arena:
        arena.region("scores", np.float32, scores.size, misalign=mis[0], role="in")
        arena.region("labels", np.uint8, labels.size, misalign=mis[1], role="in")
        arena.region("track", np.float64, len(ROWS) * W * 5, misalign=mis[2], role="out")
        arena.upload("scores", scores)
        arena.upload("labels", labels)
        ctx.score_track(arena.ptr("scores"), arena.ptr("labels"), WO, spans_of(hop, "whole"), ORIGIN, hop, W, arena.ptr("track"),
                        _lib.MEM_DEVICE)
        ctx.synchronize()
        arena.check()
        assert arena.unwritten("track") == 0
        got = arena.download("track").reshape(len(ROWS), W, 5)
    assert got.tobytes() == run(ctx, scores, labels, WO, spans_of(hop, "whole"), ORIGIN, hop, W, _lib.MEM_HOST).tobytes()


def test_argument_errors_leave_the_track_untouched(ctx, decisions):
    scores, labels = decisions
    lib, W, hop = ctx.lib, 7, 7
    spans = spans_of(hop, "whole")
    track = np.full((len(ROWS), W, 5), -7.0)
    P = lambda a: None if a is None else a.ctypes.data

    def call(c=ctx.handle, s=scores, l=labels, wo=WO, U=len(ROWS), sp=spans, origin=ORIGIN, h=hop, w=W, t=track, mem=_lib.MEM_HOST):
        return lib.f2_score_track(c, P(s), P(l), P(wo), U, P(sp), origin, h, w, P(t), mem)

    down = WO.copy()
    down[2] = down[3] + 1
    shifted = WO + 1
    neg, back = spans.copy(), spans.copy()
    neg[1] = (-1, 5)
    back[2] = (9, 8)
    far = np.array([0, 2 ** 40], np.int64)
    invalid = [dict(c=None), dict(wo=None), dict(sp=None), dict(s=None), dict(l=None), dict(t=None), dict(U=-1), dict(h=0), dict(origin=-1),
               dict(w=0), dict(wo=shifted), dict(wo=down), dict(sp=neg), dict(sp=back), dict(mem=3), dict(mem=_lib.MEM_HOST_ASYNC)]
    for kw in invalid:
        assert call(**kw) == _lib.F2_ERR_INVALID, kw
    assert call(w=65537) == _lib.F2_ERR_UNSUPPORTED
    # (nothing is read: the row count alone takes the last row's sample past int64)
    assert call(wo=far, U=1, sp=spans[:1].copy(), h=2 ** 31 - 1, origin=2 ** 62, t=track) == _lib.F2_ERR_UNSUPPORTED
    assert (track == -7.0).all()
    assert call(U=0, t=None, s=None, l=None, wo=np.zeros(1, np.int64)) == _lib.F2_OK
    assert call() == _lib.F2_OK and not (track == -7.0).any()
