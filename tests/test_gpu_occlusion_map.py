"""f2_occlusion_map: the scores and labels of an occluded evaluation reduced to the time columns of a picture, per utterance and
patch, against a NumPy / math.fsum referee of the header's definition - counts exact, the means inside the bound of any summation
order; NaN scores, bit identity between calls and memory spaces, placement between guard bands, argument errors. Rows, hops, widths
and spans are those of tests/test_gpu_score_track.py (the conditions the cases must meet are asserted on the referee alone)."""
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
KS = (1, 5)
KMAX = max(KS)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def decisions():
    """{K: (scores (n, K + 1, 2) = (1 - p, p), p uniform in [0, 1) as float32; random labels (n, K + 1))}: the K = 1 arrays are the
    first two levels of the K = 5 ones, so one referee serves both"""
    rng = np.random.default_rng(115)
    n = int(WO[-1])
    p = rng.random((n, KMAX + 1)).astype(np.float32)
    scores = np.ascontiguousarray(np.stack([np.float32(1) - p, p], axis=2))
    labels = rng.integers(0, 2, (n, KMAX + 1)).astype(np.uint8)
    return {K: (np.ascontiguousarray(scores[:, :K + 1]), np.ascontiguousarray(labels[:, :K + 1])) for K in KS}


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
    """map (U, KMAX, W, 4) with the fsum means, computed once per case; its [:, :K] is the map of the K-patch arrays"""
    key = (hop, W, kind)
    if key not in _referee:
        scores, labels = decisions[KMAX]
        spans = spans_of(hop, kind)
        out = np.full((len(ROWS), KMAX, W, 4), np.nan)
        for u, n in enumerate(ROWS):
            p = scores[WO[u]:WO[u + 1], :, 1].astype(np.float64)
            lab = labels[WO[u]:WO[u + 1]] != 0
            j0, j1 = owned_rows(n, spans[u], hop, W)
            for k in range(KMAX):
                d = p[:, k + 1] - p[:, 0]
                flip = lab[:, k + 1] != lab[:, 0]
                for x in range(W):
                    seg = d[j0[x]:j1[x]]
                    out[u, k, x, 0], out[u, k, x, 1] = len(seg), np.count_nonzero(flip[j0[x]:j1[x]])
                    if len(seg):
                        out[u, k, x, 2] = math.fsum(seg.tolist()) / len(seg)
                        out[u, k, x, 3] = math.fsum(np.abs(seg).tolist()) / len(seg)
        _referee[key] = out
    return _referee[key]


def run(ctx, scores, labels, wo, K, spans, origin, hop, W, mem, fill=-7.0):
    U = len(wo) - 1
    out = np.full((U, K, W, 4), fill)
    if mem == _lib.MEM_HOST:
        ctx.occlusion_map(scores, labels, wo, K, spans, origin, hop, W, out, mem)
        return out
    d_s, d_l, d_t = ctx.malloc(max(scores.nbytes, 8)), ctx.malloc(max(labels.nbytes, 8)), ctx.malloc(max(out.nbytes, 8))
    try:
        ctx.h2d(d_s, scores)
        ctx.h2d(d_l, labels)
        ctx.h2d(d_t, out)
        ctx.occlusion_map(d_s, d_l, wo, K, spans, origin, hop, W, d_t, mem)
        ctx.synchronize()
        ctx.d2h(out, d_t)
    finally:
        for p in (d_s, d_l, d_t):
            ctx.free(p)
    return out


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


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("hop,W,kind", CASES)
def test_map_against_the_definition(ctx, decisions, hop, W, kind, K):
    scores, labels = decisions[K]
    want = referee(decisions, hop, W, kind)[:, :K]
    spans = spans_of(hop, kind)
    got = [run(ctx, scores, labels, WO, K, spans, ORIGIN, hop, W, mem) for mem in MEMS]
    again = run(ctx, scores, labels, WO, K, spans, ORIGIN, hop, W, _lib.MEM_DEVICE)
    assert got[0].tobytes() == got[1].tobytes() == again.tobytes()          # the same bits in both memory spaces and on every call
    t = got[0]
    for c in (0, 1):
        assert np.array_equal(t[..., c], want[..., c]), c
    empty = want[..., 0] == 0
    # any order of adding `rows` float64 terms, then one division: (rows + 2) * 2^-53 * (the mean of |d|), for both means
    bound = (want[..., 0] + 2) * 2.0 ** -53 * want[..., 3]
    for c in (2, 3):
        assert np.isnan(t[..., c][empty]).all() and not np.isnan(t[..., c][~empty]).any()
        err = np.abs(t[..., c] - want[..., c])
        print(f"K {K} hop {hop} W {W} {kind} [{c}]: worst error / bound "
              f"{np.nanmax(np.where(empty, 0.0, err / np.maximum(bound, 1e-300))):.3f}")
        assert (err[~empty] <= bound[~empty]).all()


def test_one_nan_score_spoils_its_column_and_patch_only(ctx, decisions):
    K, hop, W = 5, 7, 64
    scores, labels = decisions[K]
    want = referee(decisions, hop, W, "whole")
    u, j, k = 3, 1234, 2
    j0, j1 = owned_rows(ROWS[u], spans_of(hop, "whole")[u], hop, W)
    x = int(np.flatnonzero((j0 <= j) & (j < j1))[0])
    bad = scores.copy()
    bad[WO[u] + j, k + 1, 1] = np.nan
    clean = run(ctx, scores, labels, WO, K, spans_of(hop, "whole"), ORIGIN, hop, W, _lib.MEM_DEVICE)
    for mem in MEMS:
        t = run(ctx, bad, labels, WO, K, spans_of(hop, "whole"), ORIGIN, hop, W, mem)
        assert np.isnan(t[u, k, x, 2:]).all() and np.array_equal(t[u, k, x, :2], want[u, k, x, :2])
        t[u, k, x, 2:] = clean[u, k, x, 2:]
        assert t.tobytes() == clean.tobytes()
    # a NaN at level 0 belongs to every patch of its column
    bad = scores.copy()
    bad[WO[u] + j, 0, 1] = np.nan
    t = run(ctx, bad, labels, WO, K, spans_of(hop, "whole"), ORIGIN, hop, W, _lib.MEM_DEVICE)
    assert np.isnan(t[u, :, x, 2:]).all()
    t[u, :, x, 2:] = clean[u, :, x, 2:]
    assert t.tobytes() == clean.tobytes()


def test_outputs_between_guard_bands_at_odd_alignments(ctx, decisions):
    K, hop, W = 5, 7, 300
    scores, labels = decisions[K]
    with Arena(ctx) as arena:
        arena.region("scores", np.float32, scores.size, misalign=3, role="in")
        arena.region("labels", np.uint8, labels.size, misalign=5, role="in")
        arena.region("map", np.float64, len(ROWS) * K * W * 4, misalign=7, role="out")
        arena.upload("scores", scores)
        arena.upload("labels", labels)
        ctx.occlusion_map(arena.ptr("scores"), arena.ptr("labels"), WO, K, spans_of(hop, "whole"), ORIGIN, hop, W, arena.ptr("map"),
                          _lib.MEM_DEVICE)
        ctx.synchronize()
        arena.check()
        assert arena.unwritten("map") == 0
        got = arena.download("map").reshape(len(ROWS), K, W, 4)
    assert got.tobytes() == run(ctx, scores, labels, WO, K, spans_of(hop, "whole"), ORIGIN, hop, W, _lib.MEM_HOST).tobytes()


def test_argument_errors_leave_the_map_untouched(ctx, decisions):
    K0, W, hop = 5, 7, 7
    scores, labels = decisions[K0]
    lib = ctx.lib
    spans = spans_of(hop, "whole")
    out = np.full((len(ROWS), K0, W, 4), -7.0)
    P = lambda a: None if a is None else a.ctypes.data

    def call(c=ctx.handle, s=scores, l=labels, wo=WO, U=len(ROWS), K=K0, sp=spans, origin=ORIGIN, h=hop, w=W, t=out, mem=_lib.MEM_HOST):
        return lib.f2_occlusion_map(c, P(s), P(l), P(wo), U, K, P(sp), origin, h, w, P(t), mem)

    down = WO.copy()
    down[2] = down[3] + 1
    shifted = WO + 1
    neg, back = spans.copy(), spans.copy()
    neg[1] = (-1, 5)
    back[2] = (9, 8)
    far = np.array([0, 2 ** 40], np.int64)
    invalid = [dict(c=None), dict(wo=None), dict(sp=None), dict(s=None), dict(l=None), dict(t=None), dict(U=-1), dict(h=0), dict(origin=-1),
               dict(w=0), dict(wo=shifted), dict(wo=down), dict(sp=neg), dict(sp=back), dict(mem=3), dict(mem=_lib.MEM_HOST_ASYNC),
               dict(K=0), dict(K=-1)]
    for kw in invalid:
        assert call(**kw) == _lib.F2_ERR_INVALID, kw
    assert call(w=65537) == _lib.F2_ERR_UNSUPPORTED
    assert call(K=1025) == _lib.F2_ERR_UNSUPPORTED
    # (nothing is read: the row count alone takes the last row's sample past int64)
    assert call(wo=far, U=1, sp=spans[:1].copy(), h=2 ** 31 - 1, origin=2 ** 62) == _lib.F2_ERR_UNSUPPORTED
    assert (out == -7.0).all()
    assert call(U=0, t=None, s=None, l=None, wo=np.zeros(1, np.int64)) == _lib.F2_OK
    assert call() == _lib.F2_OK and not (out == -7.0).any()
