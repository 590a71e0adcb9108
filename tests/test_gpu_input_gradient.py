"""f2_cnn_input_gradient: G = dP(rising)/dx by the backward-data chain of csrc/f2_cnn_grad.hip against the PyTorch autograd referee
(tests/saliency_referee.py, which states the acceptance rule and where its numbers come from), the profile against the float64 row
sums of the returned G, and the promises of the header: the same bits on every call, in both memory spaces and wherever a window
stands in the batch; exact zeros for a dead network; a non-finite window spoils no other."""
import numpy as np
import pytest

import saliency_referee as sr
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

IDS = ["{}x{}".format(c[2], c[3]) for c in sr.CASES]
SMALL = sr.CASES[0]      # (13, 40): odd conv2 / conv4 heights and an odd conv4 width - the pool drops rows and columns


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def gradient(ctx, model, x, mem=_lib.MEM_HOST, grad=True, profile=True, scores=True):
    """(G, profile, scores) of f2_cnn_input_gradient for x (n, rows, channels) float32 in the memory space `mem`; None where not asked"""
    n, R, C = x.shape
    out = [np.full((n, R, C), -7.0, np.float32) if grad else None, np.full((n, C, 2), -7.0) if profile else None,
           np.full((n, 2), -7.0, np.float32) if scores else None]
    h = model.handle(ctx)
    if mem == _lib.MEM_HOST:
        ctx.cnn_input_gradient(h, x, n, out[0], out[1], out[2], mem)
        return out
    d_x = ctx.malloc(x.nbytes)
    d_out = [ctx.malloc(a.nbytes) if a is not None else None for a in out]
    try:
        ctx.h2d(d_x, x)
        for d, a in zip(d_out, out):
            if a is not None:
                ctx.h2d(d, a)
        ctx.cnn_input_gradient(h, d_x, n, d_out[0], d_out[1], d_out[2], mem)
        ctx.synchronize()
        for d, a in zip(d_out, out):
            if a is not None:
                ctx.d2h(a, d)
    finally:
        for d in [d_x] + d_out:
            if d is not None:
                ctx.free(d)
    return out


@pytest.fixture(scope="module")
def small(ctx):
    """the referee of the small shape and the device's answer for its windows, computed once"""
    ref = sr.referee(*SMALL)
    return ref, gradient(ctx, ref.model, ref.x)


@pytest.mark.parametrize("case", sr.CASES, ids=IDS)
def test_gradient_against_the_referee(ctx, case):
    ref = sr.referee(*case)
    G, scores = ref.model.input_gradient(ref.x, ctx=ctx)
    assert G.dtype == np.float32 and G.shape == ref.x.shape and np.isfinite(G).all()
    quiet, beyond = sr.accept(G, ref, "device {}".format(case))
    e32 = sr.window_errors(ref.G32, ref)
    print("float32 CPU chain on the same windows: max e_w within tolerance {:.3g}".format(float(e32[e32 <= sr.TOL].max())))
    err = np.abs(scores.astype(np.float64) - ref.scores64).max()
    print("scores: max |device - float64 referee| {:.3g}".format(err))
    assert err <= 2e-5


def test_profile_is_the_float64_row_sum_of_the_returned_gradient(small):
    ref, (G, profile, _) = small
    terms = G.astype(np.float64) * ref.x.astype(np.float64)
    for k, t in enumerate((terms, np.abs(G.astype(np.float64)))):
        want = np.zeros(profile.shape[:2])
        for r in range(t.shape[1]):           # r ascending, as the header states
            want += t[:, r]
        scale = np.abs(t).sum(axis=1)
        err = np.abs(profile[..., k] - want)
        print("profile[{}]: worst error / sum of |terms| {:.3g}".format(k, float((err / np.maximum(scale, 1e-300)).max())))
        assert (err <= 1e-12 * scale).all()
    assert (profile[..., 1] >= 0).all()


def test_outputs_are_optional_and_do_not_change_each_other(ctx, small):
    ref, (G, profile, scores) = small
    x = ref.x[:40]
    only_profile = gradient(ctx, ref.model, x, grad=False, scores=False)[1]
    only_grad = gradient(ctx, ref.model, x, profile=False, scores=False)[0]
    only_scores = gradient(ctx, ref.model, x, grad=False, profile=False)[2]
    assert only_profile.tobytes() == profile[:40].tobytes()
    assert only_grad.tobytes() == G[:40].tobytes()
    assert only_scores.tobytes() == scores[:40].tobytes()


def test_same_bits_on_every_call_and_in_both_memory_spaces(ctx, small):
    ref, first = small
    again = gradient(ctx, ref.model, ref.x)
    device = gradient(ctx, ref.model, ref.x, mem=_lib.MEM_DEVICE)
    for a, b, c in zip(first, again, device):
        assert a.tobytes() == b.tobytes() == c.tobytes()


@pytest.mark.parametrize("mem", (_lib.MEM_HOST, _lib.MEM_DEVICE), ids=("host", "device"))
def test_chunking_is_invisible(ctx, small, mem):
    """4096 + 70 windows cross the host staging chunk and several chunks of the chain's scratch: the first 64 and the last 70
    windows carry the bits of calls of their own"""
    ref, _ = small
    n = 4096 + 70
    x = np.ascontiguousarray(np.random.default_rng(11).random((n,) + ref.x.shape[1:]).astype(np.float32))
    x[:64] = ref.x[:64]
    whole = gradient(ctx, ref.model, x, mem=mem)
    head = gradient(ctx, ref.model, x[:64], mem=mem)
    tail = gradient(ctx, ref.model, x[-70:], mem=mem)
    for w, h, t in zip(whole, head, tail):
        assert w[:64].tobytes() == h.tobytes()
        assert w[-70:].tobytes() == t.tobytes()
    assert whole[0][:64].tobytes() == small[1][0][:64].tobytes()


def test_dead_network_gives_exact_zeros(ctx):
    """x all zeros and a model with zero biases: every pre-activation is exactly 0, no ReLU passes, G is exactly 0 and P = 1/2"""
    _, _, rows, channels, _ = SMALL
    model = F2CNNModel.glorot(7, rows, channels, zero_bias=True)
    x = np.zeros((33, rows, channels), np.float32)
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        G, profile, scores = gradient(ctx, model, x, mem=mem)
        assert not np.isnan(G).any() and not np.isnan(profile).any()
        assert (G == 0).all() and (profile == 0).all() and (scores == 0.5).all()


def test_a_nan_window_changes_no_other_window(ctx, small):
    ref, clean = small
    bad = ref.x.copy()
    bad[77] = np.nan
    bad[200, 3, 5] = np.inf
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        got = gradient(ctx, ref.model, bad, mem=mem)
        keep = np.ones(len(bad), bool)
        keep[[77, 200]] = False
        for g, c in zip(got, clean):
            assert g[keep].tobytes() == c[keep].tobytes()


def test_argument_errors_write_nothing(ctx, small):
    ref, _ = small
    lib, h = ctx.lib, ref.model.handle(ctx)
    x = ref.x[:8]
    G = np.full(x.shape, -7.0, np.float32)
    prof = np.full((8, x.shape[2], 2), -7.0)
    sc = np.full((8, 2), -7.0, np.float32)
    P = lambda a: None if a is None else a.ctypes.data

    def call(c=ctx.handle, m=h, xx=x, n=8, mem=_lib.MEM_HOST):
        return lib.f2_cnn_input_gradient(c, m, P(xx), n, P(G), P(prof), P(sc), mem)

    for kw in (dict(c=None), dict(m=None), dict(xx=None), dict(n=-1), dict(mem=3), dict(mem=_lib.MEM_HOST_ASYNC)):
        assert call(**kw) == _lib.F2_ERR_INVALID, kw
    assert (G == -7.0).all() and (prof == -7.0).all() and (sc == -7.0).all()
    assert call(n=0, xx=None) == _lib.F2_OK and (G == -7.0).all()
    assert call() == _lib.F2_OK and not (G == -7.0).any() and not (prof == -7.0).any() and not (sc == -7.0).any()
