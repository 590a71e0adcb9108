"""f2_saliency_map: the profile rows of f2_cnn_input_gradient reduced to the time columns of a picture, per utterance and channel,
against a NumPy restatement of f2_score_track's column rule (PlottingProcessing.column_edges) - counts exact, the means to 1e-12
relative; ragged window offsets, an empty utterance, empty columns, a width above the row count; the same bits on every call and in
both memory spaces; argument errors with nothing written."""
import numpy as np
import pytest

from f2cnn_amd import _lib
from f2cnn_amd.scripts.plotting import PlottingProcessing as pp

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 37, 700, 5000)        # per utterance: ragged, one of them empty
WO = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int64)
C = 5
ORIGIN = 800
HOPS = (1, 160)
WIDTHS = (1, 7, 64)                 # 64 is above the row count of three of the utterances
MEMS = (_lib.MEM_HOST, _lib.MEM_DEVICE)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def profile():
    rng = np.random.default_rng(116)
    p = rng.standard_normal((int(WO[-1]), C, 2))
    p[..., 1] = np.abs(p[..., 1])
    return np.ascontiguousarray(p)


def spans_of(hop, kind):
    if kind == "inner":                       # a span inside the utterance: the columns outside the rows' samples stay empty
        return np.array([[790, 830]] * len(ROWS), np.int64)
    if kind == "wide":                        # a span that starts before the first row and ends far behind the last: empty columns
        return np.array([[0, 4 * ORIGIN + 3 * n * hop] for n in ROWS], np.int64)
    return np.array([[0, 2 * ORIGIN + n * hop] for n in ROWS], np.int64)


def owned_rows(n, span, hop, W):
    """(j_lo, j_hi) per column: the rows j of an utterance of n rows with lo_x <= ORIGIN + j hop < hi_x"""
    s, e = int(span[0]), int(span[1])
    if e == s:
        return np.zeros(W, np.int64), np.zeros(W, np.int64)
    lo, hi = pp.column_edges(e - s, W, s)
    t = ORIGIN + hop * np.arange(n, dtype=np.int64)
    return np.searchsorted(t, lo, side="left"), np.searchsorted(t, hi, side="left")


def restatement(profile, hop, W, kind):
    spans = spans_of(hop, kind)
    out = np.full((len(ROWS), C, W, 3), np.nan)
    for u, n in enumerate(ROWS):
        p = profile[WO[u]:WO[u + 1]]
        j0, j1 = owned_rows(n, spans[u], hop, W)
        for x in range(W):
            out[u, :, x, 0] = j1[x] - j0[x]
            if j1[x] > j0[x]:
                out[u, :, x, 1:] = p[j0[x]:j1[x]].sum(axis=0) / (j1[x] - j0[x])
    return out


def run(ctx, profile, wo, Cn, spans, origin, hop, W, mem, fill=-7.0):
    U = len(wo) - 1
    out = np.full((U, Cn, W, 3), fill)
    if mem == _lib.MEM_HOST:
        ctx.saliency_map(profile, wo, Cn, spans, origin, hop, W, out, mem)
        return out
    d_p, d_t = ctx.malloc(max(profile.nbytes, 8)), ctx.malloc(max(out.nbytes, 8))
    try:
        ctx.h2d(d_p, profile)
        ctx.h2d(d_t, out)
        ctx.saliency_map(d_p, wo, Cn, spans, origin, hop, W, d_t, mem)
        ctx.synchronize()
        ctx.d2h(out, d_t)
    finally:
        for p in (d_p, d_t):
            ctx.free(p)
    return out


@pytest.mark.parametrize("kind", ("whole", "inner", "wide"))
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("hop", HOPS)
def test_map_against_the_column_rule(ctx, profile, hop, W, kind):
    want = restatement(profile, hop, W, kind)
    spans = spans_of(hop, kind)
    got = [run(ctx, profile, WO, C, spans, ORIGIN, hop, W, mem) for mem in MEMS]
    again = run(ctx, profile, WO, C, spans, ORIGIN, hop, W, _lib.MEM_DEVICE)
    assert got[0].tobytes() == got[1].tobytes() == again.tobytes()          # the same bits in both memory spaces and on every call
    t = got[0]
    assert np.array_equal(t[..., 0], want[..., 0])
    empty = want[..., 0] == 0
    assert (t[0, :, :, 0] == 0).all() and np.isnan(t[0, :, :, 1:]).all()     # the empty utterance: {0, NaN, NaN} everywhere
    if W > 1:
        assert empty[1:].any()                                               # and empty columns in utterances that have rows
    assert (~empty).any()
    for c in (1, 2):
        assert np.isnan(t[..., c][empty]).all() and not np.isnan(t[..., c][~empty]).any()
    # relative to the largest term (the means of column [1] cancel, so not to the mean itself): any order of adding up to 5000
    # float64 terms and one division stays within 5002 * 2^-53 = 6e-13 of it
    scale = np.abs(profile).max()
    for c in (1, 2):
        err = np.abs(t[..., c] - want[..., c])[~empty]
        print(f"hop {hop} W {W} {kind} [{c}]: worst error {err.max():.3g} of scale {scale:.3g}")
        assert (err <= 1e-12 * scale).all()


def test_argument_errors_leave_the_map_untouched(ctx, profile):
    W, hop = 7, 7
    lib = ctx.lib
    spans = spans_of(hop, "whole")
    out = np.full((len(ROWS), C, W, 3), -7.0)
    P = lambda a: None if a is None else a.ctypes.data

    def call(c=ctx.handle, p=profile, wo=WO, U=len(ROWS), Cn=C, sp=spans, origin=ORIGIN, h=hop, w=W, t=out, mem=_lib.MEM_HOST):
        return lib.f2_saliency_map(c, P(p), P(wo), U, Cn, P(sp), origin, h, w, P(t), mem)

    down = WO.copy()
    down[2] = down[3] + 1
    shifted = WO + 1
    neg, back = spans.copy(), spans.copy()
    neg[1] = (-1, 5)
    back[2] = (9, 8)
    far = np.array([0, 2 ** 40], np.int64)
    invalid = [dict(c=None), dict(wo=None), dict(sp=None), dict(p=None), dict(t=None), dict(U=-1), dict(h=0), dict(origin=-1),
               dict(w=0), dict(wo=shifted), dict(wo=down), dict(sp=neg), dict(sp=back), dict(mem=3), dict(mem=_lib.MEM_HOST_ASYNC),
               dict(Cn=0), dict(Cn=-1)]
    for kw in invalid:
        assert call(**kw) == _lib.F2_ERR_INVALID, kw
    assert call(w=65537) == _lib.F2_ERR_UNSUPPORTED
    assert call(Cn=65536) == _lib.F2_ERR_UNSUPPORTED
    # (nothing is read: the row count alone takes the last row's sample past int64)
    assert call(wo=far, U=1, sp=spans[:1].copy(), h=2 ** 31 - 1, origin=2 ** 62) == _lib.F2_ERR_UNSUPPORTED
    assert (out == -7.0).all()
    assert call(U=0, t=None, p=None, wo=np.zeros(1, np.int64)) == _lib.F2_OK
    assert call() == _lib.F2_OK and not (out == -7.0).any()
