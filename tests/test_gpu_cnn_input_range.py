"""f2_cnn_forward / F2CNNModel.predict on inputs of any range (keras model.predict takes any float32 input): the split-fp16
path scales its operands for the input bound it measures (k_cnn_input_range, f2_cnn_split.h), and inputs it cannot take - inf /
NaN, or a bound that would need a scale outside the clamp - run on the float32 kernels. Every result is held against the
oracle's float64-accumulating referee as closely as the float32 kernels (option cnn_f16x3 = 0) are."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

CHUNK = 16384            # windows per chunk of a host-memory f2_cnn_forward (f2_pipeline.hip: CNN_CHUNK)
SHAPES = [(11, 128), (13, 40)]   # the weight-stationary kernels; the per-tile kernels (conv3 / conv4 on the float32 kernels)


def f32_predict(ctx, m, x):
    with ctx.options(cnn_f16x3=0):
        return m.predict(x, ctx)


def bound(ctx, m):
    return ctx.cnn_info(m.handle(ctx), "last_input_bound")


def balanced(ctx, base, x):
    """`base` with the dense2 bias moved so that the decision boundary sits at the median logit gap of x: half the windows on
    either side of it, many of them close."""
    s = f32_predict(ctx, base, x).astype(np.float64)
    gap = np.log(np.maximum(s[:, 1], 1e-300)) - np.log(np.maximum(s[:, 0], 1e-300))
    shift = float(np.median(gap[np.isfinite(gap)]))
    t = dict(base.tensors)
    t["dense2_b"] = (t["dense2_b"].astype(np.float64) + np.array([0.5 * shift, -0.5 * shift])).astype(np.float32)
    return F2CNNModel(t, base.rows, base.channels)


def models(ctx, x, seed=5):
    base = F2CNNModel.glorot(seed, x.shape[1], x.shape[2], zero_bias=False)
    return [("glorot", base), ("balanced", balanced(ctx, base, x))]


def check_against_referee(tag, m, x, got, ref32):
    """As close to the float64 referee as the float32 kernels are; labels identical wherever the referee's margin is clear."""
    assert np.isfinite(got).all(), tag
    truth = orc.cnn_forward_referee(x, dict(m.tensors))
    e_split, e_f32 = np.abs(got - truth).max(), np.abs(ref32 - truth).max()
    print(f"{tag}: max |score - referee| split {e_split:.2e}, float32 {e_f32:.2e}")
    assert e_split <= 2.0 * e_f32 + 2e-7, tag
    clear = np.abs(truth[:, 1] - truth[:, 0]) > 1e-5
    np.testing.assert_array_equal(orc.labels_from_scores(got)[clear], orc.labels_from_scores(truth)[clear], err_msg=tag)
    return truth


@pytest.mark.parametrize("rows,channels,n", [(11, 128, 500), (13, 40, 520)])
def test_large_inputs(rows, channels, n):
    """x = 100 rand: before this, the fp16 pieces overflowed and every score came back NaN."""
    ctx = _lib.default_context()
    x = (100.0 * np.random.default_rng(31).random((n, rows, channels))).astype(np.float32)
    for tag, m in models(ctx, x):
        got = m.predict(x, ctx)
        assert bound(ctx, m) == 128.0, tag
        check_against_referee(f"{rows}x{channels} {tag}", m, x, got, f32_predict(ctx, m, x))


@pytest.mark.parametrize("rows,channels", SHAPES)
def test_one_spike(rows, channels):
    """Inputs in [0, 1] and one 1e4 spike in one window. The split path's scales are the call's: with B = 2^14 set by the spike,
    the other windows' activations would sit 14 binades below them and lose the low bits of their second fp16 pieces. So a call
    whose quietest window lies more than 2^4 below B runs on the float32 kernels - bit for bit what they give."""
    ctx = _lib.default_context()
    x = np.random.default_rng(32).random((300, rows, channels)).astype(np.float32)
    x[123, rows // 2, channels // 3] = 1e4
    for tag, m in models(ctx, x):
        got = m.predict(x, ctx)
        assert bound(ctx, m) == -1.0, tag
        ref32 = f32_predict(ctx, m, x)
        np.testing.assert_array_equal(got, ref32, err_msg=tag)
        check_against_referee(f"{rows}x{channels} {tag}", m, x, got, ref32)


@pytest.mark.parametrize("rows,channels", SHAPES)
def test_mixed_sign(rows, channels):
    ctx = _lib.default_context()
    x = (50.0 * (2.0 * np.random.default_rng(33).random((300, rows, channels)) - 1.0)).astype(np.float32)
    for tag, m in models(ctx, x):
        got = m.predict(x, ctx)
        assert bound(ctx, m) == 64.0, tag
        check_against_referee(f"{rows}x{channels} {tag}", m, x, got, f32_predict(ctx, m, x))


@pytest.mark.parametrize("rows,channels", SHAPES)
def test_power_of_two_sweep(rows, channels):
    ctx = _lib.default_context()
    x0 = np.random.default_rng(34).random((200, rows, channels)).astype(np.float32)
    ms = models(ctx, x0)
    for k in (3, 7, 13, 19):
        x = x0 * np.float32(2.0 ** k)
        for tag, m in ms:
            got = m.predict(x, ctx)
            b = bound(ctx, m)
            assert b in (2.0 ** k, -1.0), (tag, k, b)     # -1: a scale would leave the clamp - the float32 kernels ran
            check_against_referee(f"{rows}x{channels} {tag} x 2^{k} (B {b:g})", m, x, got, f32_predict(ctx, m, x))


def test_host_chunks_and_device_memory():
    """Host memory: the range is measured per chunk - the first chunk keeps its B = 1 bits whatever the second holds. Device
    memory: one bound for the whole call."""
    ctx = _lib.default_context()
    rows, channels, n = 11, 128, CHUNK + 300
    rng = np.random.default_rng(35)
    x = rng.random((n, rows, channels)).astype(np.float32)
    x[CHUNK:] *= np.float32(100.0)
    m = F2CNNModel.glorot(6, rows, channels, zero_bias=False)
    got = m.predict(x, ctx)
    assert bound(ctx, m) == 128.0                      # the larger of the two chunks' bounds (1, 128)
    alone = m.predict(x[:CHUNK], ctx)
    assert bound(ctx, m) == 1.0
    np.testing.assert_array_equal(got[:CHUNK], alone)
    ref32 = f32_predict(ctx, m, x)
    check_against_referee("host chunk 2", m, x[CHUNK:], got[CHUNK:], ref32[CHUNK:])

    # a spike in the second chunk: that chunk runs on the float32 kernels (test_one_spike), the first keeps its bits
    xs = x.copy()
    xs[CHUNK:] = rng.random((n - CHUNK, rows, channels))
    xs[CHUNK + 7, 5, 64] = 1e4
    got = m.predict(xs, ctx)
    assert bound(ctx, m) == -1.0
    np.testing.assert_array_equal(got[:CHUNK], alone)
    np.testing.assert_array_equal(got[CHUNK:], f32_predict(ctx, m, xs[CHUNK:]))

    xd = (100.0 * rng.random((n, rows, channels))).astype(np.float32)
    d_x = ctx.malloc(xd.nbytes)
    d_s = ctx.malloc(n * 2 * 4)
    try:
        ctx.h2d(d_x, xd)
        ctx.cnn_forward(m.handle(ctx), d_x, n, d_s, None, _lib.MEM_DEVICE)
        dev = np.empty((n, 2), np.float32)
        ctx.d2h(dev, d_s)
    finally:
        ctx.free(d_x)
        ctx.free(d_s)
    assert bound(ctx, m) == 128.0
    pick = np.concatenate([np.arange(0, CHUNK, 64), np.arange(CHUNK, n)])   # the referee is slow: a sample of chunk 1
    check_against_referee("device memory", m, xd[pick], dev[pick], f32_predict(ctx, m, xd[pick]))


@pytest.mark.parametrize("rows,channels", SHAPES)
def test_float32_route(rows, channels):
    """Inputs the split path cannot take run on the float32 kernels: the same scores, bit for bit."""
    ctx = _lib.default_context()
    m = F2CNNModel.glorot(7, rows, channels, zero_bias=False)
    rng = np.random.default_rng(36)
    huge = (1e30 * rng.random((100, rows, channels))).astype(np.float32)
    got = m.predict(huge, ctx)
    assert bound(ctx, m) == -1.0
    np.testing.assert_array_equal(got, f32_predict(ctx, m, huge))
    x = rng.random((100, rows, channels)).astype(np.float32)
    x[40, 1, 2] = np.inf
    got = m.predict(x, ctx)
    assert bound(ctx, m) == -1.0
    np.testing.assert_array_equal(got, f32_predict(ctx, m, x))


def test_in_range_inputs_keep_their_scales():
    """x in [0, 1]: B = 1. The window tensor of an utterance through f2_cnn_forward (one range pass) gives the scores the
    `cnn eval` pipeline gives (no range pass: K3's windows lie in [0, 1]) bit for bit."""
    ctx = _lib.default_context()
    m = F2CNNModel.glorot(7, zero_bias=False)
    assert ctx.cnn_info(m.handle(ctx), "last_input_bound") == 0.0      # no call yet
    x = np.random.default_rng(37).random((300, 11, 128)).astype(np.float32)
    m.predict(x, ctx)
    assert bound(ctx, m) == 1.0

    wave = orc.synth_utterance(4321, 16000)
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, 128, 100))
    radius, step, C = 5, 1, 128
    env = np.empty((C, len(wave)))
    nb = len(wave) - (2 * radius + 1) * step
    scores = np.empty((nb, 2), np.float32)
    labels = np.empty(nb, np.uint8)
    got_nb = ctx.eval_utterance(m.handle(ctx), wave, _lib.WAVE_I16, len(wave), coefs, C, True, 50.0, _lib.FFT_F32, radius,
                                step, env, scores, labels, _lib.MEM_HOST)
    assert got_nb == nb
    win = np.empty((nb, 2 * radius + 1, C), np.float32)
    ctx.gather_windows(env, C, len(wave), None, nb, radius, step, True, win, _lib.MEM_HOST)
    assert win.min() >= 0.0 and win.max() <= 1.0
    s2 = np.empty((nb, 2), np.float32)
    l2 = np.empty(nb, np.uint8)
    ctx.cnn_forward(m.handle(ctx), win, nb, s2, l2, _lib.MEM_HOST)
    assert bound(ctx, m) == 1.0
    np.testing.assert_array_equal(s2, scores)
    np.testing.assert_array_equal(l2, labels)


def test_create_time_check_of_the_split_path():
    """f2_cnn_create holds the split path against the float32 kernels at B = 1 and B = 2^10."""
    ctx = _lib.default_context()
    for rows, channels in SHAPES:
        x = np.random.default_rng(38).random((200, rows, channels)).astype(np.float32)
        for tag, m in models(ctx, x):
            h = m.handle(ctx)
            assert ctx.cnn_info(h, "f16x3_ok") == 1.0, tag
            d = ctx.cnn_info(h, "f16x3_check_diff")
            print(f"{rows}x{channels} {tag}: f16x3_check_diff {d:.2e}")
            assert 0.0 <= d <= 1e-6, tag
