"""Referee of the training step (f2_cnn_loss_gradient, f2_trainer_*): the F2CNN network in PyTorch on the CPU with autograd, in
float64 and in float32, the summed cross-entropy, Keras' three dropout layers with masks restated in NumPy from the header's
formula, and the selection of windows that stand clear of every ReLU mask and max-pool choice.

    ref = referee(seed, xseed, rows, channels, n, candidates, drop)     (cached: the tests of one case share it and leave it unchanged)
    ref.model, ref.x, ref.y      F2CNNModel.glorot(seed, rows, channels, zero_bias=False), the n selected windows (float32) and labels
    ref.kept, ref.tried          windows kept, candidates looked at (the kept fraction)
    ref.g64, ref.g32             the gradient of the summed loss for the 12 tensors in Keras layouts, float64 and float32 chain
    ref.loss64, ref.loss32       the loss sums
    ref.z64                      (n, 2) logits of the float64 chain in training mode
    ref.margin                   (n,) the smallest |pre-activation| over all ReLU units and the smallest pool lead, masks applied

Why windows are selected: a weight gradient sums over windows, so a ReLU or pool decision that float32 rounding turns in one window
cannot be set aside afterwards. The selection uses the inputs alone - the float64 margin of a candidate at the place in the batch
it would take (its dropout masks depend on that place) - and never the device's answer: no window is excluded afterwards.

accept(grads, loss, ref) applies the acceptance rule: max|g - g64| / max|g64| <= TOL for each of the 12 tensors and for the loss.
"""
import functools
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
CASES = ((7, 9, 13, 40, 256, 1500),     # odd conv2 / conv4 heights, a partial second x-tile, the pool drops a row and a column
         (7, 9, 18, 20, 256, 1000),     # three pooled rows into dense1
         (5, 4, 11, 128, 32, 1500))     # the production shape
TENSORS = tuple(n + s for n in NAMES for s in ("_w", "_b"))
MASK = np.uint64(0xFFFFFFFF)


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


def chain(model, x, y, masks, dtype):
    """(grads (dict, Keras layouts), loss sum, logits, margin) of the network in training mode on x (n, rows, channels)"""
    import torch
    w = torch_weights(model, dtype)
    leaves = []
    for name in NAMES:
        w[name] = tuple(t.requires_grad_(True) for t in w[name])
        leaves.extend(w[name])
    xt = torch.tensor(np.asarray(x), dtype=dtype)[:, None]
    z1, z2, a2, p1 = _head(w, xt, dtype)
    z3, z4, a4, z5, logits = _tail(w, p1, masks, dtype)
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(np.asarray(y, np.int64)), reduction="sum")
    loss.backward()
    n = len(x)
    with torch.no_grad():
        margin = torch.minimum(_smallest(n, z1, z2, z3, z4, z5), torch.minimum(_pool_lead(a2), _pool_lead(a4))).numpy().astype(np.float64)
    hp2, wp2 = ((model.rows - 2) // 2 - 2) // 2, ((model.channels - 2) // 2 - 2) // 2
    g = {}
    for name in NAMES[:4]:
        g[name + "_w"] = np.transpose(w[name][0].grad.numpy(), (2, 3, 1, 0)).copy()
        g[name + "_b"] = w[name][1].grad.numpy().copy()
    g["dense1_w"] = np.transpose(w["dense1"][0].grad.numpy().reshape(516, 64, hp2, wp2), (2, 3, 1, 0)).reshape(-1, 516).copy()
    g["dense1_b"] = w["dense1"][1].grad.numpy().copy()
    g["dense2_w"] = w["dense2"][0].grad.numpy().T.copy()
    g["dense2_b"] = w["dense2"][1].grad.numpy().copy()
    return g, float(loss.detach()), logits.detach().numpy(), margin


@functools.lru_cache(maxsize=None)
def referee(seed, xseed, rows, channels, n, candidates, drop):
    import torch
    model = F2CNNModel.glorot(seed, rows, channels, zero_bias=False)
    rng = np.random.default_rng(xseed)
    cand = rng.random((candidates, rows, channels)).astype(np.float32)
    labels = rng.integers(0, 2, candidates).astype(np.uint8)
    kept, tried = select(model, cand, n, drop)
    x, y = np.ascontiguousarray(cand[kept]), np.ascontiguousarray(labels[kept])
    masks = masks_for(np.arange(n), rows, channels, drop)
    g64, loss64, z64, margin = chain(model, x, y, masks, torch.float64)
    threads = torch.get_num_threads()
    torch.set_num_threads(CHAIN_THREADS)
    try:
        g32, loss32, _, _ = chain(model, x, y, masks, torch.float32)
    finally:
        torch.set_num_threads(threads)
    assert margin.min() > MARGIN, "the selection and the chain disagree about a margin"
    for a in [x, y, z64, margin] + list(g64.values()) + list(g32.values()):
        a.setflags(write=False)
    return types.SimpleNamespace(model=model, x=x, y=y, kept=n, tried=tried, g64=g64, g32=g32, loss64=loss64, loss32=loss32, z64=z64,
                                 margin=margin, masks=masks, drop=drop)


def errors(grads, loss, ref):
    """{tensor: max|g - g64| / max|g64|} and the same for the loss"""
    e = {k: float(np.abs(np.asarray(grads[k], np.float64) - ref.g64[k]).max() / np.abs(ref.g64[k]).max()) for k in TENSORS}
    e["loss"] = abs(float(loss) - ref.loss64) / abs(ref.loss64)
    return e


def accept(grads, loss, ref, what="", tol=None):
    """Asserts the acceptance rule; prints every figure first and returns the largest."""
    tol = TOL if tol is None else tol
    e = errors(grads, loss, ref)
    print("{} kept {}/{} min margin {:.3g}: ".format(what, ref.kept, ref.tried, float(ref.margin.min())) +
          " ".join("{} {:.3g}".format(k, v) for k, v in e.items()))
    bad = {k: v for k, v in e.items() if not v <= tol}
    assert not bad, "{}: beyond {}: {}".format(what, tol, bad)
    return max(e.values())
