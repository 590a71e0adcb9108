"""Referee of the training step (f2_cnn_loss_gradient, f2_trainer_*): the F2CNN network in PyTorch on the CPU with autograd, in
float64 and in float32, the summed cross-entropy, Keras' three dropout layers with masks restated in NumPy from the header's
formula, and the selection of windows that stand clear of every ReLU mask and max-pool choice.

    ref = referee(seed, xseed, rows, channels, n, candidates, drop, dense2_gain=1.0)
                                 (cached: the tests of one case share it and leave it unchanged; dense2_gain - one factor, or a pair
                                 for the kernel and for the bias - multiplies dense2's kernel and bias to drive the softmax into
                                 saturation; no margin involves dense2, so the selection is the same)
    ref.model, ref.x, ref.y      F2CNNModel.glorot(seed, rows, channels, zero_bias=False), the n selected windows (float32) and labels
    ref.kept, ref.tried          windows kept, candidates looked at (the kept fraction)
    ref.g64, ref.g32             the gradient of the summed loss for the 12 tensors in Keras layouts, float64 and float32 chain
    ref.s64                      for the same 12 tensors the sum over windows and pixels of |input| |gradient at the pre-activation|
                                 (float64 chain): the sum of the |terms| of every element; 0 where every term is 0
    ref.loss64, ref.loss32       the loss sums
    ref.z64                      (n, 2) logits of the float64 chain in training mode
    ref.margin                   (n,) the smallest |pre-activation| over all ReLU units and the smallest pool lead, masks applied

Why windows are selected: a weight gradient sums over windows, so a ReLU or pool decision that float32 rounding turns in one window
cannot be set aside afterwards. The selection uses the inputs alone - the float64 margin of a candidate at the place in the batch
it would take (its dropout masks depend on that place) - and never the device's answer: no window is excluded afterwards.

accept(grads, loss, ref) applies the acceptance rule: max|g - g64| / max|g64| <= TOL for each of the 12 tensors and for the loss,
and exact zeros wherever ref.s64 is 0. That second rule needs no tolerance: a term vanishes only through a ReLU mask, a pool loser,
a dropped cell or a padding cell, and the selection margin makes every chain agree on all of those. It speaks for the elements the
first rule is deaf to (a dead channel, a masked cell), where garbage from a pad cell, an unused tile column or a neighbouring share
would land. There is no per-element relative bound: the float32 CPU chain's own |g32 - g64| / s64 reaches 9e-3 on elements whose
error is inherited from upstream activations (dense1_w at 18 x 20).
"""
import functools
import os
import re
import types

import numpy as np

from f2cnn_amd.model import NAMES, F2CNNModel
from saliency_referee import _pool_lead, torch_weights

MARGIN = 4e-6
# Four times (saliency_referee.TOL's factor) the largest error of the float32 CPU chain against float64 over all CASES x DROPS,
# max|g32 - g64| / max|g64| per tensor: MEASURED (tests/test_train_referee.py prints every figure and holds the chain to it)
MEASURED = 3.7e-6     # (conv3_b at 18 x 20 without dropout: 3.57e-6 and 3.67e-6 on two machines; the loss: at most 7.8e-8)
TOL = 4 * MEASURED
# Threads of the float32 chain: PyTorch splits its sums by the thread count (one thread: errors up to 1.4e-5; sixteen: 2.2e-6), so
# the count is fixed. Even so its kernels differ a little between machines: CHAIN_BOUND, what tests/test_train_referee.py holds
# the chain to, is twice MEASURED (a tensor's error moved by up to a factor of 2 between two machines; the largest one by 3 %).
CHAIN_THREADS = 8
CHAIN_BOUND = 2 * MEASURED
DROP = (0.25, 0.25, 0.5)
DROPS = ((0.0, 0.0, 0.0), DROP)
MASK_SEED, MASK_STEP = 0x123456789ABCDEF, 3
# (model seed, xseed, rows, channels, windows, candidates)
# The last four are chosen for k_wgrad_conv's task shares (a window's tasks of 64 pixels = 2 rows x 32 columns are cut into shares of
# at most WGRAD_MAX_PER = 16; layer_shares() below restates the rule) and for k_wgrad_conv1's pixel walk, whose eight runs change
# their residue at a window boundary only where rows x channels is no multiple of 8. Eight windows are enough: every window runs
# every share.
#   case       conv2: Ho x Wo, tasks -> shares         conv3                       conv4                            rows channels mod 8
#   75 x 21    73 x 19, 37 -> 13/13/11                 36 x 9, 18 -> 9/9           34 x 7, 17 -> 9/8                7
#   70 x 22    68 x 20, 34 -> 12/12/10                 34 x 10, 17 -> 9/8          32 x 8, 16 -> 16 (1024 terms)    4
#   36 x 35    34 x 33, 34 -> 12/12/10 (the second     17 x 16, 9 (odd height,     15 x 14, 8                       4
#              x-tile holds one column)                padding 1)
#   11 x 130   9 x 128, four full x-tiles, 20 -> 10/10 4 x 64, two full tiles, 4   2 x 62, 2                        6
# 75 x 21 also makes both pools drop a row or a column (H2 = 73, W2 = 19, W4 = 7). The earlier cases: one share everywhere, but conv2
# at 11 x 128 (20 -> 10/10), and rows x channels = 0 mod 8.
CASES = ((7, 9, 13, 40, 256, 1500),     # odd conv2 / conv4 heights, a partial second x-tile, the pool drops a row and a column
         (7, 9, 18, 20, 256, 1000),     # three pooled rows into dense1
         (5, 4, 11, 128, 32, 1500),     # the production shape
         (7, 9, 75, 21, 8, 6000),
         (7, 9, 70, 22, 8, 6000),
         (7, 9, 36, 35, 8, 6000),
         (7, 9, 11, 130, 8, 6000))
# 1024 + 70 selected windows with dropout: the places >= 1024 of the batch stand in the chain's second chunk (not one of CASES: with
# DROP only, and only the tests that are about the chunk use it)
CHUNK_CASE = (7, 9, 13, 40, 1094, 9000)
# Saturated softmax: CASES[0] without dropout with dense2's kernel and bias times SATURATION_GAIN = (kernel's, bias'). In the
# float64 chain at least a quarter of the windows then have |z1 - z0| > SATURATED (float32 expf(-x) is 0 from x = 104 on, so the
# losing score is exactly 0 there) and at least a quarter have |z1 - z0| < UNSATURATED; tests/test_train_referee.py asserts both
# shares. Why two factors: with the weights as drawn z1 - z0 lies between -0.143 and -0.075 for all 256 windows, the bias'
# -0.049 and the kernel's -0.094 .. -0.026, so one common factor f would have to be > 110 / 0.1183 = 930 for the first share and
# < 80 / 0.1020 = 784 for the second. A bias factor of the opposite sign takes part of what the windows have in common away:
# z1 - z0 then lies between -163 and -24 (every window decided 'falling'), 70 windows beyond 110 (33 of them labelled rising, a
# loss of about |z1 - z0| each) and 66 within 80. Chosen from the float64 logits alone.
# No window may stand near z1 = z0, and SATURATION_CLEAR says so: there d(dz)/d(z1 - z0) = s0 s1 is up to 1/4, and float32 logits
# that the gain has blown up to several hundred carry errors of 1e-4 .. 1e-3 (their ulp times the root of the number of terms;
# the activations' own rounding times the gain), so the case would measure the gain and not the kernels. From |z1 - z0| = 20 on
# s0 s1 < 2.1e-9 and such an error moves no gradient by more than 1e-12. (A pair of factors that centres z1 - z0 on 0 - 16 384
# and -20 480, |z1 - z0| from 2.2 to 590 - shows it: the float32 CPU chain reads 4.0e-6 there but 2.3e-5 at half the factors,
# and the device 3.9e-5.)
SATURATION_GAIN = (2048.0, -576.0)
SATURATED, UNSATURATED, SATURATION_CLEAR = 110.0, 80.0, 20.0
TENSORS = tuple(n + s for n in NAMES for s in ("_w", "_b"))
MASK = np.uint64(0xFFFFFFFF)


def wgrad_max_per():
    """WGRAD_MAX_PER as csrc/f2_cnn_train.hip states it"""
    import f2cnn_amd
    path = os.path.join(os.path.dirname(f2cnn_amd.__file__), "csrc", "f2_cnn_train.hip")
    with open(path) as f:
        return int(re.search(r"constexpr int WGRAD_MAX_PER = (\d+);", f.read()).group(1))


def wgrad_shares(ho, wo, max_per):
    """csrc/f2_cnn_train.hip's wgrad_shares and k_wgrad_conv's `first` / `last`, restated: the task counts of the shares of a window
    with an Ho x Wo output"""
    tpw = ((ho + 1) // 2) * ((wo + 31) // 32)
    gpw = max(1, (tpw + max_per - 1) // max_per)
    per = (tpw + gpw - 1) // gpw
    return [min(first + per, tpw) - first for first in range(0, gpw * per, per)]


def layer_shares(rows, channels, max_per):
    """{layer: shares} for the three layers of k_wgrad_conv, from the window shape"""
    h2, w2 = rows - 2, channels - 2
    hp1, wp1 = h2 // 2, w2 // 2
    return {"conv2": wgrad_shares(h2, w2, max_per), "conv3": wgrad_shares(hp1, wp1, max_per), "conv4": wgrad_shares(hp1 - 2, wp1 - 2, max_per)}


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two; -> four uint64 arrays holding the 32-bit output words"""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & MASK, n2, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def keep_scale(rate):
    return np.float32(1.0 / (1.0 - rate))


def dropout_mask(seed, step, layer, positions, per, rate):
    """(len(positions), per) float32: 0 where the element is dropped, the float32 nearest 1 / (1 - rate) where it is kept.
    Element e of the window at place b of the batch uses word e & 3 of
    Philox(counter = (e >> 2, b, layer, step & 0xffffffff), key = (seed & 0xffffffff, seed >> 32)); kept iff word 2^-32 >= rate."""
    positions = np.asarray(positions, dtype=np.uint64)
    if rate == 0:
        return np.ones((len(positions), per), np.float32)
    e = np.arange(per, dtype=np.uint64)
    words = philox4x32_10((e[None, :] >> np.uint64(2), positions[:, None], layer, step & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32))
    word = np.choose((e & np.uint64(3)).astype(np.int64)[None, :], words)
    keep = word.astype(np.float64) * 2.0 ** -32 >= rate
    return np.where(keep, keep_scale(rate), np.float32(0)).astype(np.float32)


def masks_for(positions, rows, channels, drop, seed=MASK_SEED, step=MASK_STEP):
    """the three masks of the windows at `positions` of a batch, in the library's element order: (n, Hp1, Wp1, 32), (n, Hp2, Wp2, 64), (n, 516)"""
    hp1, wp1 = (rows - 2) // 2, (channels - 2) // 2
    hp2, wp2 = (hp1 - 2) // 2, (wp1 - 2) // 2
    n = len(positions)
    return (dropout_mask(seed, step, 0, positions, hp1 * wp1 * 32, drop[0]).reshape(n, hp1, wp1, 32),
            dropout_mask(seed, step, 1, positions, hp2 * wp2 * 64, drop[1]).reshape(n, hp2, wp2, 64),
            dropout_mask(seed, step, 2, positions, 516, drop[2]))


def _nchw(mask, dtype):
    import torch
    return torch.tensor(np.ascontiguousarray(np.transpose(mask, (0, 3, 1, 2))), dtype=dtype)


def _head(w, x, dtype):
    """conv1, conv2, pool 1: the part no mask reaches -> (z1, z2, a2, p1)"""
    import torch
    F = torch.nn.functional
    z1 = F.conv2d(x, *w["conv1"], padding=1)
    z2 = F.conv2d(torch.relu(z1), *w["conv2"])
    a2 = torch.relu(z2)
    return z1, z2, a2, F.max_pool2d(a2, 2)


def _tail(w, p1, masks, dtype):
    """from the first dropout on -> (z3, z4, a4, z5, logits)"""
    import torch
    F = torch.nn.functional
    z3 = F.conv2d(p1 * _nchw(masks[0], dtype), *w["conv3"], padding=1)
    z4 = F.conv2d(torch.relu(z3), *w["conv4"])
    a4 = torch.relu(z4)
    p2 = F.max_pool2d(a4, 2) * _nchw(masks[1], dtype)
    z5 = F.linear(p2.flatten(1), *w["dense1"])
    a5 = torch.relu(z5) * torch.tensor(masks[2], dtype=dtype)
    return z3, z4, a4, z5, F.linear(a5, *w["dense2"])


def _smallest(n, *tensors):
    import torch
    return torch.stack([t.abs().reshape(n, -1).min(dim=1).values for t in tensors]).min(dim=0).values


def select(model, cand, n, drop):
    """Indices of the first n candidates whose float64 margin, at the place in the batch they take, is > MARGIN; and how many
    candidates were looked at. Greedy: the candidates that pass the mask-free part stand in line; a block of them is evaluated at
    the places it would take if all passed, the run up to the first failure is kept (with dropout a failure moves everyone behind
    it up one place, to other masks)."""
    import torch
    dt = torch.float64
    w = torch_weights(model, dt)
    rows, channels = model.rows, model.channels
    with torch.no_grad():
        line, p1s = [], []
        for s in range(0, len(cand), 250):
            x = torch.tensor(cand[s:s + 250], dtype=dt)[:, None]
            z1, z2, a2, p1 = _head(w, x, dt)
            m = torch.minimum(_smallest(len(x), z1, z2), _pool_lead(a2)).numpy()
            for j in np.flatnonzero(m > MARGIN):
                line.append(s + j)
                p1s.append(p1[j])
        kept, at, tried = [], 0, 0
        block = 24 if any(drop) else 128
        while len(kept) < n and at < len(line):
            idx = line[at:at + block]
            pos = np.arange(len(kept), len(kept) + len(idx))
            z3, z4, a4, z5, _ = _tail(w, torch.stack([p1s[at + k] for k in range(len(idx))]), masks_for(pos, rows, channels, drop), dt)
            ok = torch.minimum(_smallest(len(idx), z3, z4, z5), _pool_lead(a4)).numpy() > MARGIN
            if any(drop):
                run = int(np.argmin(ok)) if not ok.all() else len(idx)     # the leading run of passes
                take = min(run, n - len(kept))
                kept.extend(idx[:take])
                at += take if take < run or run == len(idx) else run + 1   # (skip the failure behind the run)
            else:
                for k in np.flatnonzero(ok)[:n - len(kept)]:
                    kept.append(idx[k])
                at += len(idx)
        tried = line[at - 1] + 1 if at else 0
    assert len(kept) == n, "only {} of {} windows found among {} candidates".format(len(kept), n, len(cand))
    return np.array(kept), tried


def _keras_layouts(model, conv_w, conv_b, d1w, d1b, d2w, d2b):
    """the 12 tensors in Keras layouts from four conv kernels (OIHW) and biases, dense1 (516, flat in NCHW order) and dense2 (2, 516)"""
    hp2, wp2 = ((model.rows - 2) // 2 - 2) // 2, ((model.channels - 2) // 2 - 2) // 2
    g = {}
    for name, kw, kb in zip(NAMES[:4], conv_w, conv_b):
        g[name + "_w"] = np.transpose(kw.numpy(), (2, 3, 1, 0)).copy()
        g[name + "_b"] = kb.numpy().copy()
    g["dense1_w"] = np.transpose(d1w.numpy().reshape(516, 64, hp2, wp2), (2, 3, 1, 0)).reshape(-1, 516).copy()
    g["dense1_b"] = d1b.numpy().copy()
    g["dense2_w"] = d2w.numpy().T.copy()
    g["dense2_b"] = d2b.numpy().copy()
    return g


def chain(model, x, y, masks, dtype, terms=False):
    """(grads (dict, Keras layouts), loss sum, logits, margin) of the network in training mode on x (n, rows, channels); with `terms`
    a fifth value: for every element of the 12 tensors the sum over windows and pixels of |input| |gradient at the pre-activation|"""
    import torch
    F = torch.nn.functional
    w = torch_weights(model, dtype)
    leaves = []
    for name in NAMES:
        w[name] = tuple(t.requires_grad_(True) for t in w[name])
        leaves.extend(w[name])
    xt = torch.tensor(np.asarray(x), dtype=dtype)[:, None]
    z1, z2, a2, p1 = _head(w, xt, dtype)
    z3, z4, a4, z5, logits = _tail(w, p1, masks, dtype)
    pre = (z1, z2, z3, z4, z5, logits)
    if terms:
        for z in pre:
            z.retain_grad()
    # The summed cross-entropy of two classes as softplus(u), u = z_other - z_true, in the form max(u, 0) + log1p(exp(-|u|)): the
    # same number as F.cross_entropy's, but its gradient is sigmoid(u) to full relative precision on both sides. Autograd through
    # log_softmax forms softmax - onehot, which for the true class of a window with z_true - z_other > 37 is 1 - 1 = 0 in float64
    # where the answer is -exp(-37): it would make ref.s64 call elements zero that are not. The float32 chain, which is only the
    # yardstick of float32 rounding (MEASURED), keeps F.cross_entropy and the figures measured with it.
    if dtype == torch.float64:
        rising = torch.tensor(np.asarray(y) != 0)
        u = torch.where(rising, logits[:, 0] - logits[:, 1], logits[:, 1] - logits[:, 0])
        loss = (torch.relu(u) + torch.log1p(torch.exp(-u.abs()))).sum()
    else:
        loss = F.cross_entropy(logits, torch.tensor(np.asarray(y, np.int64)), reduction="sum")
    loss.backward()
    n = len(x)
    with torch.no_grad():
        margin = torch.minimum(_smallest(n, z1, z2, z3, z4, z5), torch.minimum(_pool_lead(a2), _pool_lead(a4))).numpy().astype(np.float64)
        g = _keras_layouts(model, [w[k][0].grad for k in NAMES[:4]], [w[k][1].grad for k in NAMES[:4]], w["dense1"][0].grad,
                           w["dense1"][1].grad, w["dense2"][0].grad, w["dense2"][1].grad)
        out = g, float(loss.detach()), logits.detach().numpy(), margin
        if not terms:
            return out
        # every layer's input as _head / _tail fed it, and |dLoss/dz| of its pre-activations
        ins = (xt, torch.relu(z1), p1 * _nchw(masks[0], dtype), torch.relu(z3),
               (F.max_pool2d(a4, 2) * _nchw(masks[1], dtype)).flatten(1), torch.relu(z5) * torch.tensor(masks[2], dtype=dtype))
        ga = [z.grad.abs() for z in pre]
        conv_w = [torch.nn.grad.conv2d_weight(ins[k].abs(), w[NAMES[k]][0].shape, ga[k], padding=pad) for k, pad in enumerate((1, 0, 1, 0))]
        conv_b = [ga[k].sum(dim=(0, 2, 3)) for k in range(4)]
        s = _keras_layouts(model, conv_w, conv_b, ga[4].T @ ins[4].abs(), ga[4].sum(dim=0), ga[5].T @ ins[5].abs(), ga[5].sum(dim=0))
    return out + (s,)


@functools.lru_cache(maxsize=None)
def referee(seed, xseed, rows, channels, n, candidates, drop, dense2_gain=1.0):
    import torch
    model = F2CNNModel.glorot(seed, rows, channels, zero_bias=False)
    if dense2_gain != 1.0:
        gain_w, gain_b = dense2_gain if isinstance(dense2_gain, tuple) else (dense2_gain, dense2_gain)
        t = dict(model.tensors)
        t["dense2_w"], t["dense2_b"] = t["dense2_w"] * np.float32(gain_w), t["dense2_b"] * np.float32(gain_b)
        model = F2CNNModel(t, rows, channels)
    rng = np.random.default_rng(xseed)
    cand = rng.random((candidates, rows, channels)).astype(np.float32)
    labels = rng.integers(0, 2, candidates).astype(np.uint8)
    kept, tried = select(model, cand, n, drop)
    x, y = np.ascontiguousarray(cand[kept]), np.ascontiguousarray(labels[kept])
    masks = masks_for(np.arange(n), rows, channels, drop)
    g64, loss64, z64, margin, s64 = chain(model, x, y, masks, torch.float64, terms=True)
    threads = torch.get_num_threads()
    torch.set_num_threads(CHAIN_THREADS)
    try:
        g32, loss32, _, _ = chain(model, x, y, masks, torch.float32)
    finally:
        torch.set_num_threads(threads)
    assert margin.min() > MARGIN, "the selection and the chain disagree about a margin"
    for a in [x, y, z64, margin] + list(g64.values()) + list(g32.values()) + list(s64.values()):
        a.setflags(write=False)
    return types.SimpleNamespace(model=model, x=x, y=y, kept=n, tried=tried, g64=g64, g32=g32, s64=s64, loss64=loss64, loss32=loss32,
                                 z64=z64, margin=margin, masks=masks, drop=drop)


def zero_terms(ref):
    """how many elements of the 12 tensors have no nonzero term at all (ref.s64 is 0)"""
    return int(sum((ref.s64[k] == 0).sum() for k in TENSORS))


def errors(grads, loss, ref):
    """{tensor: max|g - g64| / max|g64|} and the same for the loss"""
    e = {k: float(np.abs(np.asarray(grads[k], np.float64) - ref.g64[k]).max() / np.abs(ref.g64[k]).max()) for k in TENSORS}
    e["loss"] = abs(float(loss) - ref.loss64) / abs(ref.loss64)
    return e


def accept(grads, loss, ref, what="", tol=None):
    """Asserts the acceptance rule and the exact zeros; prints every figure first and returns the largest error."""
    tol = TOL if tol is None else tol
    e = errors(grads, loss, ref)
    stray = {k: int(np.count_nonzero(np.asarray(grads[k])[ref.s64[k] == 0])) for k in TENSORS}
    print("{} kept {}/{} min margin {:.3g}: ".format(what, ref.kept, ref.tried, float(ref.margin.min())) +
          " ".join("{} {:.3g}".format(k, v) for k, v in e.items()) +
          "; {} elements without a nonzero term, {} of them not 0".format(zero_terms(ref), sum(stray.values())))
    for k in TENSORS:      # (of ref.s64 itself: no sum is larger than the sum of its |terms|)
        assert (np.abs(ref.g64[k]) <= ref.s64[k] * (1 + 1e-9)).all(), "{}: |g64| above the sum of |terms| in {}".format(what, k)
    bad = {k: v for k, v in e.items() if not v <= tol}
    assert not bad, "{}: beyond {}: {}".format(what, tol, bad)
    stray = {k: v for k, v in stray.items() if v}
    assert not stray, "{}: nonzero where every term is 0 (elements per tensor): {}".format(what, stray)
    return max(e.values())
