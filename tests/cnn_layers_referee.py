"""Referee of f2_cnn_layers: the F2CNN network in PyTorch on the CPU without autograd, in float64 and in float32, down to the two
activations behind the scores, and the per-element error measure the GPU tests hold every route of the forward pass to.

    ref = referee(rows, channels, n, kind)       (cached: the tests of one shape share it and leave it unchanged)
    ref.model, ref.x        F2CNNModel.glorot(7, rows, channels, zero_bias=False) and its inputs, see inputs()
    ref.pooled64 / 32       (n, flat): conv4 + ReLU + max-pool flattened in (pooled row, pooled column, channel) order - the row order
                            of dense1_w - by the float64 / the float32 chain
    ref.dense64 / 32        (n, 516): dense1 after ReLU
    ref.scores64 / 32       (n, 2): the softmax

The measure, per window and per layer:  e_w = max_i |got_i - ref64_i| / max_i |ref64_i|.  ReLU and max-pool are continuous, so no
element is exempt. A route passes with every e_w <= its tolerance (check()).
"""
import functools
import types

import numpy as np

import saliency_referee
from f2cnn_amd.model import F2CNNModel

# (rows, channels, n) of tests/test_gpu_cnn_layers.py. Shapes the weight-stationary kernels take ...
WS_CASES = ((10, 18, 33), (11, 18, 97), (10, 35, 33), (11, 36, 33), (11, 66, 33), (11, 68, 33), (11, 70, 33), (11, 128, 193), (11, 403, 9))
# ... and shapes they refuse: one past their width limit, too narrow for them, and pooled heights other than four. 13 x 76 (pooled
# 5 x 37) gives the layer-by-layer forward a second x-tile: five conv3 columns and one pooled conv4 column in it, an odd last conv3
# row pair and a conv4 row the pool drops.
OFF_WS_CASES = ((11, 404, 9), (11, 16, 33), (13, 40, 33), (12, 21, 33), (14, 24, 33), (18, 20, 33), (13, 76, 9))
# the shapes that also run with inputs up to 2^10 (kind "big")
BIG_CASES = ((11, 70, 33), (13, 40, 33))
ALL = tuple((c, "unit") for c in WS_CASES + OFF_WS_CASES) + tuple((c, "big") for c in BIG_CASES)

# TOL32 is four times the largest e_w of the float32 CPU chain against the float64 chain over every (case, input kind) in ALL, both
# layers: 6.70e-7 (dense1 of 13 x 40, the same at 1, 4 and 8 threads; tests/test_cnn_layers_referee.py prints it and holds the chain
# to TOL32 / 4). The factor 4 is the one saliency_referee.TOL uses for the same purpose.
TOL32 = 2.68e-6
# The split-fp16 routes claim to be "as close to the truth as the float32 kernels are" within a factor 2
# (tests/test_gpu_windows_cnn.py: test_cnn_split_path_scales_follow_the_weights)
TOL_SPLIT = 2 * TOL32
T34 = 30   # conv4 output columns per tile of the fused conv3 / conv4 kernels (csrc/f2_cnn_dims.h)


def dims(rows, channels):
    hp1, wp1 = (rows - 2) // 2, (channels - 2) // 2
    return types.SimpleNamespace(Hp1=hp1, Wp1=wp1, Hp2=(hp1 - 2) // 2, Wp2=(wp1 - 2) // 2, flat=(hp1 - 2) // 2 * ((wp1 - 2) // 2) * 64)


def inputs(rows, channels, n, kind):
    """"unit": default_rng(3).random float32 with the first 8 windows replaced by zeros plus shifted impulses (every tap and padding
    edge; the impulses reach 3.8, so the split routes run with the scales of B = 4). "big": the random windows alone, times 2^10 -
    the scales of B = 2^10. (The impulse windows are left out there on purpose: f2_cnn_forward sends a call whose quietest window
    lies more than four binades under a bound above 2^4 to the float32 kernels, and the all-zero window is such a window.)"""
    x = np.random.default_rng(3).random((n, rows, channels)).astype(np.float32)
    if kind == "big":
        return x * np.float32(1024.0)
    assert kind == "unit"
    x[:8] = 0.0
    for i in range(1, 8):
        x[i, (i * 5) % rows, (i * 37) % channels] = 1.0 + 0.4 * i
    return x


def chain(model, x, dtype):
    """(pooled (n, flat) in (h, w, c) order, dense1 after ReLU (n, 516), scores (n, 2)) of the network on x in `dtype`, numpy"""
    import torch
    F = torch.nn.functional
    w = saliency_referee.torch_weights(model, dtype)
    with torch.no_grad():
        a = torch.tensor(np.asarray(x), dtype=dtype)[:, None]
        a = torch.relu(F.conv2d(a, *w["conv1"], padding=1))
        a = F.max_pool2d(torch.relu(F.conv2d(a, *w["conv2"])), 2)
        a = torch.relu(F.conv2d(a, *w["conv3"], padding=1))
        p2 = F.max_pool2d(torch.relu(F.conv2d(a, *w["conv4"])), 2)              # (n, 64, Hp2, Wp2)
        d1 = torch.relu(F.linear(p2.flatten(1), *w["dense1"]))
        scores = torch.softmax(F.linear(d1, *w["dense2"]), dim=1)
        pooled = p2.permute(0, 2, 3, 1).reshape(p2.shape[0], -1)
    return pooled.numpy().copy(), d1.numpy().copy(), scores.numpy().copy()


@functools.lru_cache(maxsize=None)
def referee(rows, channels, n, kind="unit"):
    import torch
    model = F2CNNModel.glorot(7, rows, channels, zero_bias=False)
    x = inputs(rows, channels, n, kind)
    p64, d64, s64 = chain(model, x, torch.float64)
    p32, d32, s32 = chain(model, x, torch.float32)
    for a in (x, p64, d64, s64, p32, d32, s32):
        a.setflags(write=False)
    return types.SimpleNamespace(model=model, x=x, rows=rows, channels=channels, pooled64=p64, dense64=d64, scores64=s64, pooled32=p32,
                                 dense32=d32, scores32=s32)


def window_errors(got, ref64):
    """e_w of every window: (n,) float64"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    return np.abs(got - ref64).max(axis=1) / np.abs(ref64).max(axis=1)


def dense1_of(pooled, model):
    """dense1 after ReLU from a pooled array in (h, w, c) order, in numpy float64"""
    t = model.tensors
    return np.maximum(np.asarray(pooled, np.float64) @ t["dense1_w"].astype(np.float64) + t["dense1_b"].astype(np.float64), 0.0)


def where(layer, got, ref64, rows, channels):
    """the worst element of the worst window of a layer, in words"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    e = window_errors(got, ref64)
    w = int(np.argmax(np.where(np.isfinite(e), e, np.inf)))
    i = int(np.argmax(np.abs(got[w] - ref64[w])))
    if layer == "dense1":
        return "window {}, dense unit {}: got {!r}, float64 {!r}".format(w, i, got[w, i], ref64[w, i])
    d = dims(rows, channels)
    h, col, c = i // (d.Wp2 * 64), i // 64 % d.Wp2, i % 64
    return "window {}, pooled row {}, pooled column {} (conv4 columns {}-{}, column tile {} of {}), channel {}: got {!r}, float64 {!r}".format(
        w, h, col, 2 * col, 2 * col + 1, 2 * col // T34, (2 * d.Wp2 + T34 - 1) // T34, c, got[w, i], ref64[w, i])


def check(layer, got, ref64, tol, rows, channels, what=""):
    """Asserts e_w <= tol for every window of `layer` ("pooled" / "dense1"); prints and returns the largest e_w."""
    got = np.asarray(got)
    assert got.shape == ref64.shape, (what, layer, got.shape, ref64.shape)
    e = window_errors(got, ref64)
    worst = float(e.max()) if np.all(np.isfinite(e)) else float("nan")
    print("{} {}: worst e_w {:.3g} (tolerance {:.3g})".format(what, layer, worst, tol))
    assert np.all(e <= tol), "{} {}: {} of {} windows beyond {:.3g}, worst e_w {:.3g} at {}".format(
        what, layer, int((~(e <= tol)).sum()), len(e), tol, worst, where(layer, got, ref64, rows, channels))
    return worst
