"""f2_cnn_loss_gradient: the gradient of the summed cross-entropy for the 12 weight tensors by the recorded forward in training
mode, the backward chain and the weight-gradient kernels of csrc/f2_cnn_train.hip, against the PyTorch autograd referee
(tests/train_referee.py, which states the acceptance rule, the window selection and where the tolerance comes from), and the
promises of the header: the same bits on every call and in both memory spaces, an index that only gathers, sums that are the
float64 sums of their pieces, masks that follow (seed, step, place) also past the first chunk of the chain's scratch and past the
first piece a host call stages, any nonzero label rising, a saturated softmax, exact zeros for a dead network and - in every
comparison with the referee - wherever every term of an element is zero."""
import ctypes

import numpy as np
import pytest

import train_referee as tr
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel, tensor_shapes

pytestmark = pytest.mark.gpu

IDS = ["{}x{}".format(c[2], c[3]) for c in tr.CASES]
SMALL = tr.CASES[0]
NODROP = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def blank(model):
    return {k: np.full(shp, -7.0, np.float32) for k, shp in tensor_shapes(model.rows, model.channels).items() if k in tr.TENSORS}


def loss_gradient(ctx, model, x, y, index=None, drop=NODROP, seed=tr.MASK_SEED, step=tr.MASK_STEP, mem=_lib.MEM_HOST, grads=True, loss=True):
    """(grads dict or None, (loss sum, correct) or None) of f2_cnn_loss_gradient in the memory space `mem`"""
    h = model.handle(ctx)
    m = len(x) if index is None else len(index)
    out = blank(model) if grads else None
    if mem == _lib.MEM_HOST:
        tally = ctx.cnn_loss_gradient(h, x, y, index, m, drop, seed, step, None if out is None else [out[k] for k in tr.TENSORS], mem, want_loss=loss)
        return out, tally
    bufs = [ctx.malloc(x.nbytes), ctx.malloc(max(y.nbytes, 1))]
    d_index = None
    d_out = None
    try:
        ctx.h2d(bufs[0], x)
        ctx.h2d(bufs[1], y)
        if index is not None:
            d_index = ctx.malloc(max(index.nbytes, 8))
            bufs.append(d_index)
            ctx.h2d(d_index, index)
        if out is not None:
            d_out = [ctx.malloc(out[k].nbytes) for k in tr.TENSORS]
            bufs.extend(d_out)
            for d, k in zip(d_out, tr.TENSORS):
                ctx.h2d(d, out[k])
        tally = ctx.cnn_loss_gradient(h, bufs[0], bufs[1], d_index, m, drop, seed, step, d_out, mem, want_loss=loss)
        ctx.synchronize()
        if out is not None:
            for d, k in zip(d_out, tr.TENSORS):
                ctx.d2h(out[k], d)
    finally:
        for d in bufs:
            ctx.free(d)
    return out, tally


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in tr.TENSORS)


@pytest.fixture(scope="module")
def small(ctx):
    """the referee of the small shape with dropout and the device's answer for its windows, computed once"""
    ref = tr.referee(*SMALL, tr.DROP)
    return ref, loss_gradient(ctx, ref.model, ref.x, ref.y, drop=tr.DROP)


@pytest.mark.parametrize("drop", tr.DROPS, ids=("nodrop", "drop"))
@pytest.mark.parametrize("case", tr.CASES, ids=IDS)
def test_gradient_against_the_referee(ctx, case, drop):
    ref = tr.referee(*case, drop)
    grads, (loss, correct) = loss_gradient(ctx, ref.model, ref.x, ref.y, drop=drop)
    assert all(np.isfinite(g).all() for g in grads.values())
    tr.accept(ref.g32, ref.loss32, ref, "float32 CPU chain {} {}".format(case, drop))
    tr.accept(grads, loss, ref, "device {} {}".format(case, drop))
    decided = np.abs(ref.z64[:, 1] - ref.z64[:, 0]) > 1e-4
    want = int(((ref.z64[:, 1] > ref.z64[:, 0]) == (ref.y != 0)).sum())
    print("correct {} of {}, referee {} ({} undecided)".format(correct, len(ref.y), want, int((~decided).sum())))
    assert abs(correct - want) <= int((~decided).sum())


def test_same_bits_on_every_call_and_in_both_memory_spaces(ctx, small):
    ref, (first, tally) = small
    again, tally2 = loss_gradient(ctx, ref.model, ref.x, ref.y, drop=tr.DROP)
    device, tally3 = loss_gradient(ctx, ref.model, ref.x, ref.y, drop=tr.DROP, mem=_lib.MEM_DEVICE)
    assert same_bits(first, again) and same_bits(first, device)
    assert tally == tally2 == tally3


@pytest.mark.parametrize("mem", (_lib.MEM_HOST, _lib.MEM_DEVICE), ids=("host", "device"))
def test_index_gives_the_bits_of_the_gathered_windows(ctx, small, mem):
    ref, (first, tally) = small
    rng = np.random.default_rng(3)
    n = len(ref.x)
    perm = rng.permutation(n).astype(np.int64)
    back = np.argsort(perm).astype(np.int64)                      # x[perm][back] is x: the call on the shuffled array, index undoing it
    got, t = loss_gradient(ctx, ref.model, np.ascontiguousarray(ref.x[perm]), np.ascontiguousarray(ref.y[perm]), index=back, drop=tr.DROP, mem=mem)
    assert same_bits(first, got) and t == tally
    sub = rng.integers(0, n, 45).astype(np.int64)                 # a subset with repeats
    sub[7] = sub[3]
    a, ta = loss_gradient(ctx, ref.model, ref.x, ref.y, index=sub, drop=tr.DROP, mem=mem)
    b, tb = loss_gradient(ctx, ref.model, np.ascontiguousarray(ref.x[sub]), np.ascontiguousarray(ref.y[sub]), drop=tr.DROP)
    assert same_bits(a, b) and ta == tb


@pytest.mark.parametrize("m", (1, 33))
def test_batch_is_the_float64_sum_of_its_windows(ctx, small, m):
    """without dropout a window's contribution does not depend on its place: the gradient of m windows against the float64 sum of
    the device's own m one-window gradients, within 2^-23 sum |terms| elementwise"""
    ref, _ = small
    x, y = ref.x[:m], ref.y[:m]
    whole, (loss, correct) = loss_gradient(ctx, ref.model, x, y)
    total = {k: np.zeros(whole[k].shape) for k in tr.TENSORS}
    mag = {k: np.zeros(whole[k].shape) for k in tr.TENSORS}
    lsum, csum = 0.0, 0
    for j in range(m):
        one, (l1, c1) = loss_gradient(ctx, ref.model, x[j:j + 1], y[j:j + 1])
        for k in tr.TENSORS:
            total[k] += one[k].astype(np.float64)
            mag[k] += np.abs(one[k].astype(np.float64))
        lsum, csum = lsum + l1, csum + c1
    for k in tr.TENSORS:
        err = np.abs(whole[k].astype(np.float64) - total[k])
        print("m={} {}: worst error / (2^-23 sum |terms|) {:.3g}".format(m, k, float((err / np.maximum(2.0 ** -23 * mag[k], 1e-300)).max())))
        assert (err <= 2.0 ** -23 * mag[k]).all(), k
    assert correct == csum and abs(loss - lsum) <= 1e-12 * lsum


def test_chunk_crossing(ctx):
    """1024 + 70 windows: the call works through two chunks of its scratch; against the float64 sum of the device's gradients of
    the two pieces, within 2^-23 (|g_a| + |g_b|) elementwise"""
    model = F2CNNModel.glorot(SMALL[0], SMALL[2], SMALL[3], zero_bias=False)
    rng = np.random.default_rng(11)
    x = rng.random((1094, SMALL[2], SMALL[3])).astype(np.float32)
    y = rng.integers(0, 2, 1094).astype(np.uint8)
    whole, (loss, correct) = loss_gradient(ctx, model, x, y)
    a, (la, ca) = loss_gradient(ctx, model, x[:1024], y[:1024])
    b, (lb, cb) = loss_gradient(ctx, model, x[1024:], y[1024:])
    for k in tr.TENSORS:
        a64, b64 = a[k].astype(np.float64), b[k].astype(np.float64)
        err = np.abs(whole[k].astype(np.float64) - (a64 + b64))
        bound = 2.0 ** -23 * (np.abs(a64) + np.abs(b64))
        print("{}: worst error / bound {:.3g}".format(k, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), k
    assert correct == ca + cb and abs(loss - (la + lb)) <= 1e-12 * loss
    device, t = loss_gradient(ctx, model, x, y, mem=_lib.MEM_DEVICE)
    assert same_bits(whole, device) and t == (loss, correct)


def test_dropout_and_index_past_the_first_chunk(ctx):
    """CHUNK_CASE: 1094 selected windows with dropout, so the windows at the places 1024 .. 1093 stand in the chain's second chunk.
    The referee pins their masks to the header's formula (place b = b0 + s of the batch, not of the chunk); the device-memory call
    and the calls on the shuffled arrays with the index that undoes the shuffle (the device index and the host gather, both offset
    by the chunk) give the host-memory call's bits."""
    ref = tr.referee(*tr.CHUNK_CASE, tr.DROP)
    n = len(ref.x)
    assert n > 1024
    first, tally = loss_gradient(ctx, ref.model, ref.x, ref.y, drop=tr.DROP)
    assert all(np.isfinite(g).all() for g in first.values())
    tr.accept(first, tally[0], ref, "device {} {}".format(tr.CHUNK_CASE, tr.DROP))
    device, td = loss_gradient(ctx, ref.model, ref.x, ref.y, drop=tr.DROP, mem=_lib.MEM_DEVICE)
    assert same_bits(first, device) and td == tally
    perm = np.random.default_rng(5).permutation(n).astype(np.int64)
    back = np.argsort(perm).astype(np.int64)
    assert (back[1024:] != np.arange(1024, n)).any() and (back[:1024] >= 1024).any()      # windows cross the chunk boundary both ways
    xp, yp = np.ascontiguousarray(ref.x[perm]), np.ascontiguousarray(ref.y[perm])
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        got, t = loss_gradient(ctx, ref.model, xp, yp, index=back, drop=tr.DROP, mem=mem)
        assert same_bits(first, got) and t == tally, mem


def test_past_the_first_host_piece(ctx):
    """4100 windows with dropout: the host-memory call stages a piece of 4096 and one of 4 (places 4096 + 0 ..), the device-memory
    call works through five chunks of the chain's scratch in one launch sequence (places 0 + 0 .. 4096): the same bits and tallies,
    also with a reversing index on the reversed arrays (the host gather `index[s + j]` past the first piece)"""
    model = F2CNNModel.glorot(SMALL[0], SMALL[2], SMALL[3], zero_bias=False)
    rng = np.random.default_rng(13)
    n = 4100
    x = rng.random((n, SMALL[2], SMALL[3])).astype(np.float32)
    y = rng.integers(0, 2, n).astype(np.uint8)
    host, th = loss_gradient(ctx, model, x, y, drop=tr.DROP)
    device, td = loss_gradient(ctx, model, x, y, drop=tr.DROP, mem=_lib.MEM_DEVICE)
    assert all(np.isfinite(g).all() and g.any() for g in host.values())
    assert same_bits(host, device) and th == td
    rev = np.arange(n - 1, -1, -1, dtype=np.int64)
    turned, tt = loss_gradient(ctx, model, np.ascontiguousarray(x[::-1]), np.ascontiguousarray(y[::-1]), index=rev, drop=tr.DROP)
    assert same_bits(host, turned) and tt == th


@pytest.mark.parametrize("mem", (_lib.MEM_HOST, _lib.MEM_DEVICE), ids=("host", "device"))
def test_any_nonzero_label_is_rising(ctx, small, mem):
    ref, (first, tally) = small
    assert set(np.unique(ref.y)) == {0, 1}
    for label in (2, 255):
        y = np.where(ref.y != 0, label, 0).astype(np.uint8)
        got, t = loss_gradient(ctx, ref.model, ref.x, y, drop=tr.DROP, mem=mem)
        assert same_bits(first, got) and t == tally, label


def test_saturated_softmax(ctx):
    """dense2 times SATURATION_GAIN: more than a quarter of the windows have |z1 - z0| > 110, where float32 expf underflows and the
    losing score is exactly 0 - the regime dz = rising ? -s0 : s1 was written for -, more than a quarter < 80, none < 20. Half of
    either group is decided against its label and costs about |z1 - z0| a window, unclipped, so the loss is part of the rule as ever."""
    ref = tr.referee(*SMALL, NODROP, dense2_gain=tr.SATURATION_GAIN)
    gap = np.abs(ref.z64[:, 1] - ref.z64[:, 0])
    assert (gap > tr.SATURATED).sum() >= len(gap) / 4 and (gap < tr.UNSATURATED).sum() >= len(gap) / 4
    tr.accept(ref.g32, ref.loss32, ref, "float32 CPU chain, dense2 x {}".format(tr.SATURATION_GAIN), tol=tr.CHAIN_BOUND)
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        grads, (loss, correct) = loss_gradient(ctx, ref.model, ref.x, ref.y, mem=mem)
        assert all(np.isfinite(g).all() for g in grads.values()) and np.isfinite(loss)
        tr.accept(grads, loss, ref, "device, dense2 x {}, memory space {}".format(tr.SATURATION_GAIN, mem))
        decided = gap > 1e-2                                       # (float32 logits of this size are good to about 1e-3)
        want = int(((ref.z64[:, 1] > ref.z64[:, 0]) == (ref.y != 0)).sum())
        assert abs(correct - want) <= int((~decided).sum())


def test_masks_follow_seed_step_and_rate(ctx, small):
    ref, (first, tally) = small
    x, y = ref.x[:64], ref.y[:64]
    base, tb = loss_gradient(ctx, ref.model, x, y)
    other, to = loss_gradient(ctx, ref.model, x, y, seed=99, step=12345)
    assert same_bits(base, other) and tb == to                     # rate 0 draws nothing
    d0, _ = loss_gradient(ctx, ref.model, x, y, drop=tr.DROP, seed=5, step=1)
    d1, _ = loss_gradient(ctx, ref.model, x, y, drop=tr.DROP, seed=5, step=2)
    d2, _ = loss_gradient(ctx, ref.model, x, y, drop=tr.DROP, seed=6, step=1)
    d3, _ = loss_gradient(ctx, ref.model, x, y, drop=tr.DROP, seed=5, step=1 + 2 ** 32)    # step & 0xffffffff
    again, _ = loss_gradient(ctx, ref.model, x, y, drop=tr.DROP, seed=5, step=1)
    assert same_bits(d0, again) and same_bits(d0, d3)
    assert not same_bits(d0, d1) and not same_bits(d0, d2) and not same_bits(d0, base)


def test_dead_network_gives_exact_zeros(ctx):
    model = F2CNNModel.glorot(3, SMALL[2], SMALL[3], zero_bias=True)
    m = 37
    x = np.zeros((m, SMALL[2], SMALL[3]), np.float32)
    y = (np.arange(m) % 2).astype(np.uint8)
    grads, (loss, correct) = loss_gradient(ctx, model, x, y, drop=tr.DROP)
    for k in tr.TENSORS:
        if k.endswith("_w"):
            assert not grads[k].any(), k
    assert abs(loss - m * np.log(2.0)) <= 1e-12 * m
    assert correct == int((y == 0).sum())                          # ties decide 'falling'


def test_outputs_are_optional_and_do_not_change_each_other(ctx, small):
    ref, (first, tally) = small
    only_grads, none = loss_gradient(ctx, ref.model, ref.x, ref.y, drop=tr.DROP, loss=False)
    none_grads, only_tally = loss_gradient(ctx, ref.model, ref.x, ref.y, drop=tr.DROP, grads=False)
    assert none is None and none_grads is None
    assert same_bits(first, only_grads) and only_tally == tally
    h = ref.model.handle(ctx)
    rates = (ctypes.c_double * 3)(*tr.DROP)
    hits = ctypes.c_int64(-1)
    ctx.check(ctx.lib.f2_cnn_loss_gradient(ctx.handle, h, ref.x.ctypes.data, ref.y.ctypes.data, None, len(ref.x), rates, tr.MASK_SEED, tr.MASK_STEP,
                                           None, None, ctypes.byref(hits), _lib.MEM_HOST))
    assert hits.value == tally[1]
    zero, tz = loss_gradient(ctx, ref.model, ref.x[:0], ref.y[:0])
    assert all(not g.any() for g in zero.values()) and tz == (0.0, 0)


def test_argument_errors_write_nothing(ctx, small):
    ref, _ = small
    h = ref.model.handle(ctx)
    x, y = ref.x[:8], ref.y[:8]
    out = blank(ref.model)
    ptrs = (ctypes.c_void_p * 12)(*[out[k].ctypes.data for k in tr.TENSORS])
    rates = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    loss, hits = ctypes.c_double(-7.0), ctypes.c_int64(-7)

    def call(ctx_h=ctx.handle, cnn=h, xp=x.ctypes.data, yp=y.ctypes.data, index=None, m=8, drop=rates, grads=ptrs, mem=_lib.MEM_HOST):
        return ctx.lib.f2_cnn_loss_gradient(ctx_h, cnn, xp, yp, index, m, drop, 0, 0, grads, ctypes.byref(loss), ctypes.byref(hits), mem)

    neg = np.array([0, 1, -1, 2, 3, 4, 5, 6], np.int64)
    holed = (ctypes.c_void_p * 12)(*[out[k].ctypes.data if k != "conv3_b" else None for k in tr.TENSORS])
    bad = [call(ctx_h=None), call(cnn=None), call(xp=None), call(yp=None), call(m=-1), call(drop=None), call(mem=7), call(mem=_lib.MEM_HOST_ASYNC),
           call(drop=(ctypes.c_double * 3)(0.0, 1.0, 0.0)), call(drop=(ctypes.c_double * 3)(-0.1, 0.0, 0.0)),
           call(drop=(ctypes.c_double * 3)(0.0, 0.0, float("nan"))), call(index=neg.ctypes.data), call(grads=holed)]
    assert bad == [_lib.F2_ERR_INVALID] * len(bad)
    assert all((g == -7.0).all() for g in out.values()) and loss.value == -7.0 and hits.value == -7
    assert call() == _lib.F2_OK and loss.value > 0


def test_input_gradient_keeps_its_bits_around_a_training_call(ctx, small):
    """f2_cnn_input_gradient and f2_cnn_loss_gradient share the context's gradient scratch"""
    ref, _ = small
    x = ref.x[:50]
    before = ref.model.input_gradient(x, ctx=ctx)
    loss_gradient(ctx, ref.model, ref.x, ref.y, drop=tr.DROP)
    after = ref.model.input_gradient(x, ctx=ctx)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
