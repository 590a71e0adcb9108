"""Referee of the input gradient (f2_cnn_input_gradient): the F2CNN network in PyTorch on the CPU with autograd, in float64 and
in float32, and the margin that says how close a window stands to a ReLU mask or a max-pool choice that rounding could turn.

    ref = referee(seed, xseed, rows, channels, n)      (cached: the tests of one shape share it and leave it unchanged)
    ref.model, ref.x          F2CNNModel.glorot(seed, rows, channels, zero_bias=False), default_rng(xseed).random((n, rows, channels)) f32
    ref.G64, ref.G32          dP(rising)/dx per window by the float64 and by the float32 chain, (n, rows, channels)
    ref.P64, ref.scores64     P(rising) (n,) and the softmax scores (n, 2) of the float64 chain
    ref.margin                (n,) float64: the smallest of |pre-activation| over all ReLU units and of the lead of each pool winner
                              over its runner-up where the winner is > 0 (float64 chain)

accept(G, ref) applies the acceptance rule: e_w = max|G - G64| / max|G64| <= TOL for every window, except windows whose margin is
<= MARGIN (a mask or pool decision at the float32 rounding level), which may be at most CAP of the batch.
"""
import functools
import types

import numpy as np

from f2cnn_amd.model import F2CNNModel

TOL = 5e-6       # four times the largest no-flip error of the float32 CPU chain against float64 (1.3e-6 of max|G|)
MARGIN = 1e-5
CAP = 0.02       # one flipped window in 128 was the most the float32 CPU chain showed: under 1 %
# (seed, xseed, rows, channels, n) of the GPU tests; tests/test_saliency_referee.py holds the float32 CPU chain to the rule on them
# The two tall shapes are those of train_referee.CASES, where the training step reuses this backward chain (k_conv3x3_f32) with many row
# pairs per window. At these sizes every window's margin is <= MARGIN, so the margin excuses nothing and excludes nothing: what binds
# is CAP and TOL - at most one window of 64 may lie beyond TOL (the float32 CPU chain: 0 of 64 at either shape, largest e_w 5.5e-7).
# A failure here without one in test_gpu_loss_gradient.py's cases of the same shapes places a fault in k_conv3x3_f32, not in the
# weight-gradient kernels.
CASES = ((7, 9, 13, 40, 256), (7, 9, 10, 100, 128), (5, 4, 11, 128, 128), (7, 9, 18, 20, 128),   # (18 x 20: three pooled rows into dense1)
         (7, 9, 75, 21, 64), (7, 9, 36, 35, 64))


def torch_weights(model, dtype):
    """The model's Keras-layout tensors as Conv2d (OIHW) / Linear (out, in; NCHW flatten) weights"""
    import torch
    t = model.tensors
    hp2, wp2 = ((model.rows - 2) // 2 - 2) // 2, ((model.channels - 2) // 2 - 2) // 2
    w = {}
    for name in ("conv1", "conv2", "conv3", "conv4"):
        w[name] = (torch.tensor(np.transpose(t[name + "_w"], (3, 2, 0, 1)).copy(), dtype=dtype), torch.tensor(t[name + "_b"], dtype=dtype))
    w1 = t["dense1_w"].reshape(hp2, wp2, 64, 516)
    w["dense1"] = (torch.tensor(np.transpose(w1, (3, 2, 0, 1)).reshape(516, -1).copy(), dtype=dtype), torch.tensor(t["dense1_b"], dtype=dtype))
    w["dense2"] = (torch.tensor(t["dense2_w"].T.copy(), dtype=dtype), torch.tensor(t["dense2_b"], dtype=dtype))
    return w


def _pool_lead(a):
    """per window, the smallest lead of a 2 x 2 block's winner over its runner-up among the blocks whose winner is > 0"""
    import torch
    n, c, h, w = a.shape
    b = a[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, -1, 4)
    top = torch.sort(b, dim=2, descending=True).values
    lead = torch.where(top[:, :, 0] > 0, top[:, :, 0] - top[:, :, 1], torch.full_like(top[:, :, 0], float("inf")))
    return lead.min(dim=1).values


def chain(model, x, dtype):
    """(G, scores, margin) of the network on x (n, rows, channels) in `dtype`, as numpy arrays"""
    import torch
    F = torch.nn.functional
    w = torch_weights(model, dtype)
    xt = torch.tensor(np.asarray(x), dtype=dtype)[:, None].requires_grad_(True)
    z1 = F.conv2d(xt, *w["conv1"], padding=1)
    z2 = F.conv2d(torch.relu(z1), *w["conv2"])
    a2 = torch.relu(z2)
    p1 = F.max_pool2d(a2, 2)
    z3 = F.conv2d(p1, *w["conv3"], padding=1)
    z4 = F.conv2d(torch.relu(z3), *w["conv4"])
    a4 = torch.relu(z4)
    p2 = F.max_pool2d(a4, 2)
    z5 = F.linear(p2.flatten(1), *w["dense1"])
    scores = torch.softmax(F.linear(torch.relu(z5), *w["dense2"]), dim=1)
    scores[:, 1].sum().backward()     # the windows are independent: each gets the gradient of its own P
    with torch.no_grad():
        n = xt.shape[0]
        margin = torch.stack([z.abs().reshape(n, -1).min(dim=1).values for z in (z1, z2, z3, z4, z5)] + [_pool_lead(a2), _pool_lead(a4)]).min(dim=0).values
    return xt.grad[:, 0].numpy(), scores.detach().numpy(), margin.numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def referee(seed, xseed, rows, channels, n):
    import torch
    model = F2CNNModel.glorot(seed, rows, channels, zero_bias=False)
    x = np.random.default_rng(xseed).random((n, rows, channels)).astype(np.float32)
    G64, s64, margin = chain(model, x, torch.float64)
    G32, _, _ = chain(model, x, torch.float32)
    for a in (x, G64, G32, s64, margin):
        a.setflags(write=False)
    return types.SimpleNamespace(model=model, x=x, G64=G64, G32=G32, scores64=s64, P64=s64[:, 1], margin=margin)


def window_errors(G, ref):
    n = len(ref.x)
    num = np.abs(np.asarray(G, np.float64) - ref.G64).reshape(n, -1).max(axis=1)
    return num / np.abs(ref.G64).reshape(n, -1).max(axis=1)


def accept(G, ref, what=""):
    """Asserts the acceptance rule for G against ref; prints and returns (largest no-flip error, windows beyond TOL)."""
    e = window_errors(G, ref)
    assert np.all(np.isfinite(e)), what
    beyond = e > TOL
    quiet = float(e[~beyond].max()) if (~beyond).any() else 0.0
    print("{} max e_w within tolerance {:.3g}, median {:.3g}, beyond {}: {} of {} (margins {})".format(
        what, quiet, float(np.median(e)), TOL, int(beyond.sum()), len(e), np.array2string(ref.margin[beyond], precision=2)))
    assert np.all(ref.margin[beyond] <= MARGIN), "{}: window(s) {} beyond {} with errors {} and margins {} above {}".format(
        what, np.flatnonzero(beyond & (ref.margin > MARGIN)), TOL, e[beyond & (ref.margin > MARGIN)], ref.margin[beyond & (ref.margin > MARGIN)], MARGIN)
    assert beyond.sum() <= CAP * len(e), "{}: {} of {} windows beyond {}".format(what, int(beyond.sum()), len(e), TOL)
    return quiet, int(beyond.sum())
