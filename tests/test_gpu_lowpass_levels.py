"""f2_lowpass_levels: the stand-alone first-order low-pass of envelopes in memory, at K cutoffs and as a copy in one pass.
Small ragged batches with odd lengths (rows start at odd 8-byte offsets) around every carry boundary of the kernel - the pair,
the wave of 64 pairs, the 4096-sample segment - held row by row against orc.low_pass_filter, on raw bits against the input (the
copy level) and against themselves (alone / in a batch / K = 1 / K = 5 / a second call). Through the C ABI via ctypes.

The bound of 1e-12 (per-row max-norm relative to max |x| of the row) is derived, not tuned: a CPU emulation of the blocked float64
scan against scipy.signal.lfilter on 131 072-sample rows gave 2e-16 .. 3e-15 for these cutoffs and blocks of 64 / 512 / 2048; the
bound leaves ~300x for the device's fma contraction and the formation of the powers of q."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib

pytestmark = pytest.mark.gpu

C = 3
S = 4096                                     # samples per segment of k_lowpass_levels
CUTOFFS = (0.5, 50.0, 3999.0, 4000.0, 7900.0)   # q = 0.9998 (every carry path matters) ... a1 = 0 ... q < 0
LENGTHS = (63, 1, 0, 65, 2, 64, S - 1, S + 1, S, 2 * S + 1)
BOUND = 1e-12
FILL = 0x5A


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def offsets_of(lengths):
    o = np.zeros(len(lengths) + 1, np.int64)
    o[1:] = np.cumsum(lengths)
    return o


def rows_of(flat, offsets, b):
    """the (C, n_b) block of utterance b in a ragged buffer"""
    n = int(offsets[b + 1] - offsets[b])
    return flat[C * offsets[b]:C * offsets[b + 1]].reshape(C, n)


def raw_levels(ctx, env, offsets, B, nchan, cutoffs, k, levels, mem_space=_lib.MEM_HOST):
    p = lambda a: None if a is None else a.ctypes.data
    return ctx.lib.f2_lowpass_levels(ctx.handle, p(env), p(offsets), B, nchan, p(cutoffs), k, p(levels), mem_space)


def levels_of(ctx, env, offsets, cutoffs):
    cut = np.array(cutoffs, np.float64)
    out = np.empty((len(cut) + 1, env.size), np.float64)
    bits(out)[...] = FILL
    rc = raw_levels(ctx, env, offsets, len(offsets) - 1, C, cut, len(cut), out)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return out


def make_input(kind, lengths):
    rng = np.random.default_rng(5)
    offsets = offsets_of(lengths)
    env = rng.standard_normal(C * int(offsets[-1]))            # signed: nothing assumes positive data
    if kind == "loud then quiet":
        # utterance 0 ends 1e6 times louder than utterance 1 begins: state leaking across the boundary shows at once
        r = rows_of(env, offsets, 0)
        r[:, r.shape[1] // 2:] *= 1e6
    elif kind == "step":
        # a step exactly on the first segment boundary of the longest row, on a quiet floor
        b = int(np.argmax(lengths))
        r = rows_of(env, offsets, b)
        r[:] = 1e-3 * r
        r[:, S:] += 1.0
    return env, offsets


def worst_error(levels, env, offsets, cutoffs):
    worst = 0.0
    for b in range(len(offsets) - 1):
        x = rows_of(env, offsets, b)
        if x.shape[1] == 0:
            continue
        for l, cutoff in enumerate(cutoffs):
            y = rows_of(levels[l], offsets, b)
            for c in range(C):
                err = np.abs(y[c] - orc.low_pass_filter(x[c], cutoff)).max() / np.abs(x[c]).max()
                worst = max(worst, float(err))
                assert err <= BOUND, (b, c, cutoff, float(err))
    return worst


@pytest.mark.parametrize("cutoffs", [(0.5,), CUTOFFS], ids=["K=1", "K=5"])
@pytest.mark.parametrize("kind,lengths", [("noise", LENGTHS), ("loud then quiet", (S + 1, S + 1, 65)), ("step", (65, 2 * S + 1, 1))])
def test_levels_are_the_oracles_low_pass(ctx, kind, lengths, cutoffs):
    env, offsets = make_input(kind, lengths)
    levels = levels_of(ctx, env, offsets, cutoffs)
    assert np.array_equal(bits(levels[len(cutoffs)]), bits(env))               # the copy level, bit for bit
    assert np.isfinite(levels).all()
    print("max error / max |x| over the rows:", worst_error(levels, env, offsets, cutoffs))


def test_a_row_above_131072_samples_walks_the_same_segments(ctx):
    env, offsets = make_input("noise", (131075, 3))
    levels = levels_of(ctx, env, offsets, (0.5, 7900.0))
    assert np.array_equal(bits(levels[2]), bits(env))
    print("max error / max |x| over the rows:", worst_error(levels, env, offsets, (0.5, 7900.0)))


def test_a_rows_bits_depend_on_the_row_and_its_cutoff_alone(ctx):
    env, offsets = make_input("noise", LENGTHS)
    full = levels_of(ctx, env, offsets, CUTOFFS)
    again = levels_of(ctx, env, offsets, CUTOFFS)
    assert np.array_equal(bits(full), bits(again))                               # a second call
    b = LENGTHS.index(2 * S + 1)
    alone = np.ascontiguousarray(rows_of(env, offsets, b)).reshape(-1)
    o1 = offsets_of((2 * S + 1,))
    for l, cutoff in enumerate(CUTOFFS):
        one = levels_of(ctx, alone, o1, (cutoff,))                               # alone in the batch, K = 1
        assert np.array_equal(bits(one[0]), bits(rows_of(full[l], offsets, b).reshape(-1))), cutoff
    swapped = levels_of(ctx, env, offsets, CUTOFFS[::-1])                        # another place among the cutoffs
    assert np.array_equal(bits(swapped[:5][::-1]), bits(full[:5]))
    # one channel of the row as a C = 1 batch: another place in memory, another parity of the row start
    single = np.empty((2, 2 * S + 1))
    rc = raw_levels(ctx, np.ascontiguousarray(rows_of(env, offsets, b)[1]), o1, 1, 1, np.array([0.5]), 1, single)
    assert rc == _lib.F2_OK
    assert np.array_equal(bits(single[0]), bits(rows_of(full[0], offsets, b)[1]))


def test_empty_batches(ctx):
    out = np.empty(4)
    bits(out)[...] = FILL
    assert raw_levels(ctx, None, np.zeros(1, np.int64), 0, C, np.array([50.0]), 1, None) == _lib.F2_OK
    assert raw_levels(ctx, None, np.zeros(3, np.int64), 2, C, np.array([50.0]), 1, out) == _lib.F2_OK
    assert (bits(out) == FILL).all()


@pytest.mark.parametrize("case", ["K=0", "K=65", "cutoffs NULL", "cutoff nan", "cutoff inf", "cutoff 0", "cutoff 8000", "C=0", "B<0",
                                  "offsets NULL", "offsets[0]=1", "offsets decreasing", "env NULL", "levels NULL", "mem_space"])
def test_bad_arguments_leave_the_output_alone(ctx, case):
    env, offsets = make_input("noise", (65, 2, 63))
    cut, k, nchan, nb, mem, want = np.array([50.0, 5.0]), 2, C, 3, _lib.MEM_HOST, _lib.F2_ERR_INVALID
    out = np.empty((3, env.size))
    bits(out)[...] = FILL
    dst = out
    if case == "K=0":
        k = 0
    elif case == "K=65":
        cut, k, want = np.full(65, 50.0), 65, _lib.F2_ERR_UNSUPPORTED
    elif case == "cutoffs NULL":
        cut = None
    elif case.startswith("cutoff "):
        cut[1] = {"nan": np.nan, "inf": np.inf, "0": 0.0, "8000": 8000.0}[case.split()[1]]
    elif case == "C=0":
        nchan = 0
    elif case == "B<0":
        nb = -1
    elif case == "offsets NULL":
        offsets = None
    elif case == "offsets[0]=1":
        offsets = offsets.copy()
        offsets[0] = 1
    elif case == "offsets decreasing":
        offsets = offsets.copy()
        offsets[2] = offsets[1] - 1
    elif case == "env NULL":
        env = None
    elif case == "levels NULL":
        dst = None
    else:
        mem = 7
    assert raw_levels(ctx, env, offsets, nb, nchan, cut, k, dst, mem) == want, case
    assert (bits(out) == FILL).all(), case
