"""f2_lowpass_pick: the first-order low-pass of envelopes in memory with one cutoff per utterance, or none. Utterance b is held, on
raw bytes, against block cutoff_of[b] of f2_lowpass_levels on the same input - in host memory, in device memory out of place and in
device memory in place - and against itself in another batch order, with another K and beside other cutoffs. Row lengths stand on
the carry boundaries of the kernel: the pair, the wave of 64 pairs (128 samples), the block of 512, the 4096-sample segment; with
C = 3 and odd lengths the rows start at odd 8-byte offsets. Through the C ABI via ctypes.

The bound against scipy is that of tests/test_gpu_lowpass_levels.py (derived there: 1e-12 per row, max-norm relative to max |x|);
it is not tuned here."""
import numpy as np
import pytest
from scipy.signal import butter, lfilter

from f2cnn_amd import _lib

pytestmark = pytest.mark.gpu

C = 3
LENGTHS = (0, 1, 2, 129, 513, 4095, 4096, 4097, 8193)
CUTOFFS = (5.0, 50.0, 5000.0)                  # the last: q < 0
K = len(CUTOFFS)
# every level, the unfiltered one included, at short and at long rows
PICKS = {"a": (0, 1, 2, 3, 0, 1, 2, 3, 0), "b": (3, 2, 1, 0, 2, 3, 0, 1, 2)}
BOUND = 1e-12
FILL = 0x5A
HOST, DEV = _lib.MEM_HOST, _lib.MEM_DEVICE


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


def block(flat, offsets, b):
    """the C * n_b values of utterance b in a ragged buffer"""
    return flat[C * offsets[b]:C * offsets[b + 1]]


def ptr(a):
    return None if a is None else a if isinstance(a, int) else a.ctypes.data


def raw_pick(ctx, env, offsets, B, nchan, cutoffs, k, cutoff_of, filtered, mem_space=HOST):
    return ctx.lib.f2_lowpass_pick(ctx.handle, ptr(env), ptr(offsets), B, nchan, ptr(cutoffs), k, ptr(cutoff_of), ptr(filtered), mem_space)


def pick(ctx, env, offsets, cutoffs, cutoff_of, where="host"):
    """f2_lowpass_pick in host memory, in device memory out of place ("device") or in device memory in place ("in place")"""
    cut = None if cutoffs is None else np.array(cutoffs, np.float64)
    lev = None if cutoff_of is None else np.array(cutoff_of, np.int32)
    k, B = 0 if cut is None else len(cut), len(offsets) - 1
    out = np.empty(env.size)
    bits(out)[...] = FILL
    if where == "host":
        rc = raw_pick(ctx, env, offsets, B, C, cut, k, lev, out)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        return out
    d_env, d_out = ctx.malloc(env.nbytes), ctx.malloc(env.nbytes)
    try:
        ctx.h2d(d_env, env)
        ctx.h2d(d_out, out)
        dst = d_env if where == "in place" else d_out
        rc = raw_pick(ctx, d_env, offsets, B, C, cut, k, lev, dst, DEV)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        ctx.synchronize()
        ctx.d2h(out, dst)
        if where == "device":                                       # the input of an out-of-place call stays
            back = np.empty(env.size)
            ctx.d2h(back, d_env)
            assert np.array_equal(bits(back), bits(env))
    finally:
        ctx.free(d_env)
        ctx.free(d_out)
    return out


@pytest.fixture(scope="module")
def case(ctx):
    """the batch and its levels by f2_lowpass_levels: computed once, only read"""
    offsets = offsets_of(LENGTHS)
    env = np.random.default_rng(47).standard_normal(C * int(offsets[-1]))   # signed: nothing assumes positive data
    levels = np.empty((K + 1, env.size))
    ctx.lowpass_levels(env, offsets, len(LENGTHS), C, CUTOFFS, levels, HOST)
    assert np.array_equal(bits(levels[K]), bits(env))
    for a in (offsets, env, levels):
        a.setflags(write=False)
    return env, offsets, levels


@pytest.mark.parametrize("where", ["host", "device", "in place"])
@pytest.mark.parametrize("which", sorted(PICKS))
def test_an_utterance_is_its_level_of_the_sweep(ctx, case, which, where):
    env, offsets, levels = case
    got = pick(ctx, env, offsets, CUTOFFS, PICKS[which], where)
    for b, l in enumerate(PICKS[which]):
        assert np.array_equal(bits(block(got, offsets, b)), bits(block(levels[l], offsets, b))), (b, l)


def test_the_bits_do_not_depend_on_the_batch_on_k_or_on_the_other_cutoffs(ctx, case):
    env, offsets, levels = case
    B = len(LENGTHS)
    # the batch in reverse order
    order = list(range(B))[::-1]
    lens = [LENGTHS[b] for b in order]
    renv = np.concatenate([block(env, offsets, b) for b in order])
    roff = offsets_of(lens)
    of = PICKS["a"]
    got = pick(ctx, renv, roff, CUTOFFS, [of[b] for b in order], "in place")
    for i, b in enumerate(order):
        assert np.array_equal(bits(block(got, roff, i)), bits(block(levels[of[b]], offsets, b))), b
    # K = 1: every utterance at 50 Hz; then 50 Hz as level 2 of 4 between other cutoffs
    one = pick(ctx, env, offsets, (50.0,), [0] * B, "device")
    assert np.array_equal(bits(one), bits(levels[1]))
    among = pick(ctx, env, offsets, (7.0, 3000.0, 50.0, 0.5), [2] * B, "host")
    assert np.array_equal(bits(among), bits(levels[1]))


@pytest.mark.parametrize("where", ["host", "device"])
def test_without_a_stage_the_call_copies(ctx, case, where):
    env, offsets, _ = case
    for cutoffs, of in ((CUTOFFS, None), (None, PICKS["a"]), (None, None), ((), None)):
        assert np.array_equal(bits(pick(ctx, env, offsets, cutoffs, of, where)), bits(env)), (cutoffs, of)


@pytest.mark.parametrize("of", [(K,) * len(LENGTHS), None], ids=["every utterance unfiltered", "no stage"])
def test_unfiltered_in_place_writes_nothing(ctx, case, of):
    """a buffer of poison (NaNs with a payload, which a filter would not hand back) is byte for byte as it was"""
    _, offsets, _ = case
    poison = np.full(C * int(offsets[-1]), 0x7FF8DEAD0000BEEF, np.uint64).view(np.float64)
    assert np.array_equal(bits(pick(ctx, poison, offsets, CUTOFFS, of, "in place")), bits(poison))


def test_against_scipy(ctx, case):
    env, offsets, _ = case
    B = len(LENGTHS)
    worst = 0.0
    for l, cutoff in enumerate(CUTOFFS):
        got = pick(ctx, env, offsets, CUTOFFS, [l] * B, "in place")
        b_, a_ = butter(1, cutoff / 8000)
        for b, n in enumerate(LENGTHS):
            if n == 0:
                continue
            x, y = block(env, offsets, b).reshape(C, n), block(got, offsets, b).reshape(C, n)
            for c in range(C):
                err = float(np.abs(y[c] - lfilter(b_, a_, x[c])).max() / np.abs(x[c]).max())
                worst = max(worst, err)
                print("cutoff", cutoff, "utterance", b, "channel", c, "error / max |x|", err)
                assert err <= BOUND, (cutoff, b, c, err)
    print("max error / max |x| over the rows:", worst)


def test_empty_batches(ctx):
    out = np.empty(4)
    bits(out)[...] = FILL
    cut, lev = np.array([50.0]), np.zeros(2, np.int32)
    assert raw_pick(ctx, None, np.zeros(1, np.int64), 0, C, cut, 1, lev, None) == _lib.F2_OK
    assert raw_pick(ctx, None, np.zeros(3, np.int64), 2, C, cut, 1, lev, out) == _lib.F2_OK
    assert (bits(out) == FILL).all()


@pytest.mark.parametrize("case_name,names", [
    ("K<0", "K=-1"), ("K=65", "65 cutoffs"), ("cutoffs NULL", "cutoff_hz is NULL"), ("cutoff nan", "cutoff_hz[1]"),
    ("cutoff inf", "cutoff_hz[1]"), ("cutoff 0", "cutoff_hz[1]"), ("cutoff 8000", "cutoff_hz[1]"), ("level -1", "utterance 2"),
    ("level K+1", "utterance 2"), ("C=0", ""), ("B<0", ""), ("offsets NULL", ""), ("offsets[0]=1", ""), ("offsets decreasing", ""),
    ("env NULL", ""), ("filtered NULL", ""), ("mem_space", "")])
def test_bad_arguments_leave_the_output_alone(ctx, case_name, names):
    offsets = offsets_of((65, 2, 63))
    env = np.random.default_rng(3).standard_normal(C * int(offsets[-1]))
    cut, k, nchan, nb, mem, want = np.array([50.0, 5.0]), 2, C, 3, HOST, _lib.F2_ERR_INVALID
    lev = np.array([0, 2, 1], np.int32)
    out = np.empty(env.size)
    bits(out)[...] = FILL
    dst = out
    if case_name == "K<0":
        k = -1
    elif case_name == "K=65":
        cut, k, want = np.full(65, 50.0), 65, _lib.F2_ERR_UNSUPPORTED
    elif case_name == "cutoffs NULL":
        cut = None
    elif case_name.startswith("cutoff "):
        cut[1] = {"nan": np.nan, "inf": np.inf, "0": 0.0, "8000": 8000.0}[case_name.split()[1]]
    elif case_name == "level -1":
        lev[2] = -1
    elif case_name == "level K+1":
        lev[2] = 3
    elif case_name == "C=0":
        nchan = 0
    elif case_name == "B<0":
        nb = -1
    elif case_name == "offsets NULL":
        offsets = None
    elif case_name == "offsets[0]=1":
        offsets = offsets.copy()
        offsets[0] = 1
    elif case_name == "offsets decreasing":
        offsets = offsets.copy()
        offsets[2] = offsets[1] - 1
    elif case_name == "env NULL":
        env = None
    elif case_name == "filtered NULL":
        dst = None
    else:
        mem = 7
    assert raw_pick(ctx, env, offsets, nb, nchan, cut, k, lev, dst, mem) == want, case_name
    assert names in ctx.lib.f2_last_error(ctx.handle).decode(), ctx.lib.f2_last_error(ctx.handle).decode()
    assert (bits(out) == FILL).all(), case_name
