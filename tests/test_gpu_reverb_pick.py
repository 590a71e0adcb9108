"""f2_reverb_pick: a ragged batch with one impulse response per utterance, in the layout of the waves. Utterance lengths around
the output tile of k_reverb_pick (an empty utterance, one sample, a tile less one, a tile, a tile and one, three tiles), responses
of one tap, of a tap chunk and one, and longer than most utterances, and every (utterance, room) pair, held
 - against numpy.convolve(x, h)[:n] bit for bit where every partial sum is an integer below 2^53 (the independent reference),
 - against its level of f2_reverb_levels on raw bytes (int16 / float64 input, host / device memory),
 - against the bound of tests/test_gpu_reverb_levels.py on float data,
 - against itself: alone / in the batch, another place in the batch, other rooms around it, a second call.
Through the C ABI via ctypes, as tests/test_gpu_reverb_levels.py."""
import numpy as np
import pytest

import speechlike
from f2cnn_amd import _lib
from f2cnn_amd.reverb import SyntheticRIR

pytestmark = pytest.mark.gpu

BLK, TC = _lib.REVERB_BLOCK, _lib.REVERB_TAP_CHUNK
LENGTHS = (0, 1, BLK - 1, BLK, BLK + 1, 3000)
TAPS = (1, TC + 1, 2500)
B, K = len(LENGTHS), len(TAPS)
ROOMS = [tuple((b + shift) % (K + 1) for b in range(B)) for shift in range(K + 1)]     # every (utterance, room) pair once
FILL = 0x5A
I16, F64 = _lib.WAVE_I16, _lib.WAVE_F64
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


def pack(rirs):
    return (np.concatenate(rirs).astype(np.float64) if len(rirs) else np.zeros(0)), offsets_of([len(h) for h in rirs])


def p(a):
    return None if a is None else (a if isinstance(a, int) else a.ctypes.data)


def raw_pick(ctx, wave, dtype, offsets, nb, rir, rir_offsets, k, room_of, wet, mem_space=HOST):
    return ctx.lib.f2_reverb_pick(ctx.handle, p(wave), dtype, p(offsets), nb, p(rir), p(rir_offsets), k, p(room_of), p(wet), mem_space)


def pick(ctx, wave, offsets, rirs, room_of, mem_space=HOST):
    """(total) float64 of one call, pre-filled so that an element left out shows; device calls go through buffers of their own"""
    rir, ro = pack(rirs)
    room = None if room_of is None else np.asarray(room_of, np.int32)
    out = np.empty(int(offsets[-1]), np.float64)
    bits(out)[...] = FILL
    dtype = I16 if wave.dtype == np.int16 else F64
    nb = len(offsets) - 1
    if mem_space == HOST or not len(out):
        rc = raw_pick(ctx, wave, dtype, offsets, nb, rir if len(rir) else None, ro, len(rirs), room, out, mem_space)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        return out
    d_wave, d_out = ctx.malloc(wave.nbytes), ctx.malloc(out.nbytes)
    try:
        ctx.h2d(d_wave, wave)
        ctx.memset(d_out, FILL, out.nbytes)
        rc = raw_pick(ctx, d_wave, dtype, offsets, nb, rir if len(rir) else None, ro, len(rirs), room, d_out, DEV)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        ctx.synchronize()
        ctx.d2h(out, d_out)
    finally:
        ctx.free(d_wave)
        ctx.free(d_out)
    return out


def levels_of(ctx, wave, offsets, rirs):
    rir, ro = pack(rirs)
    out = np.empty((len(rirs) + 1, int(offsets[-1])), np.float64)
    bits(out)[...] = FILL
    dtype = I16 if wave.dtype == np.int16 else F64
    rc = ctx.lib.f2_reverb_levels(ctx.handle, p(wave), dtype, p(offsets), len(offsets) - 1, p(rir), p(ro), len(rirs), p(out), HOST)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return out


def reference(x, h):
    return np.convolve(x.astype(np.float64), h)[:len(x)] if len(x) else np.zeros(0)


def cut(flat, offsets, b):
    return flat[int(offsets[b]):int(offsets[b + 1])]


@pytest.fixture(scope="module")
def int_case():
    """int16 samples over the full range (the extremes included) and integer taps in [-8, 8]: every product and every partial
    sum is an integer of magnitude below 3000 * 32768 * 8 < 8e8 < 2^53 (checked here), so any summation order gives the same
    float64"""
    rng = np.random.default_rng(21)
    offsets = offsets_of(LENGTHS)
    wave = rng.integers(-32768, 32768, int(offsets[-1])).astype(np.int16)
    wave[int(offsets[5]):int(offsets[5]) + 2] = (-32768, 32767)
    rirs = [rng.integers(-8, 9, t).astype(np.float64) for t in TAPS]
    for h in rirs:
        h[0] = h[0] or 1.0
    for b in range(B):
        x = np.abs(cut(wave, offsets, b).astype(np.float64))
        if len(x):
            assert max(np.convolve(x, np.abs(h))[:len(x)].max() for h in rirs) < 8e8
    wave.setflags(write=False)
    return wave, offsets, rirs


@pytest.fixture(scope="module")
def float_rirs():
    """float taps, so that a changed order of the sum would show"""
    rirs = [SyntheticRIR(1.0, t, seed=3, level=l) for l, t in enumerate(TAPS)]
    assert [len(h) for h in rirs] == list(TAPS)
    return rirs


@pytest.fixture(scope="module")
def float_levels(ctx, int_case, float_rirs):
    """the sweep's levels of the int16 batch under the float responses: computed once, shared, never written to"""
    wave, offsets, _ = int_case
    out = levels_of(ctx, wave, offsets, float_rirs)
    out.setflags(write=False)
    return out


def test_integer_data_is_numpys_convolution_bit_for_bit(ctx, int_case):
    wave, offsets, rirs = int_case
    for room_of in ROOMS:
        got = pick(ctx, wave, offsets, rirs, room_of)
        for b, l in enumerate(room_of):
            x = cut(wave, offsets, b)
            # (+ 0.0: an exact integer sum has one float64 but for a zero's sign; the accumulator starts from +0)
            want = x.astype(np.float64) if l == K else reference(x, rirs[l]) + 0.0
            assert np.array_equal(bits(cut(got, offsets, b)), bits(want)), (room_of, b)


@pytest.mark.parametrize("n", [1, 3, BLK + 1])
def test_every_tap_count_up_to_sixteen_is_numpys_convolution_bit_for_bit(ctx, n):
    """sixteen utterances of n samples, utterance b in a room of b + 1 taps: 1 .. 16 taps are every combination of the walk's paired
    turns (0 .. 2), its single step (0 / 1) and its 0 .. 3 last taps; BLK + 1 samples have a full tile and a tile of one output, 1
    and 3 samples a lane with fewer outputs than it owns. Integer data as in int_case: sums below 16 * 8 * 32768 < 2^53"""
    rng = np.random.default_rng([24, n])
    offsets = offsets_of((n,) * 16)
    wave = rng.integers(-32768, 32768, 16 * n).astype(np.int16)
    rirs = [rng.integers(-8, 9, t).astype(np.float64) for t in range(1, 17)]
    got = pick(ctx, wave, offsets, rirs, range(16))
    for b, h in enumerate(rirs):
        assert np.array_equal(bits(cut(got, offsets, b)), bits(reference(cut(wave, offsets, b), h) + 0.0)), (n, len(h))


@pytest.mark.parametrize("dtype,mem", [(I16, HOST), (F64, HOST), (I16, DEV), (F64, DEV)])
def test_every_utterance_is_its_level_of_the_sweep(ctx, int_case, float_rirs, float_levels, dtype, mem):
    wave, offsets, _ = int_case
    src = wave if dtype == I16 else wave.astype(np.float64)
    for room_of in ROOMS:
        got = pick(ctx, src, offsets, float_rirs, room_of, mem)
        for b, l in enumerate(room_of):
            assert np.array_equal(bits(cut(got, offsets, b)), bits(float_levels[l, int(offsets[b]):int(offsets[b + 1])])), (room_of, b)


def test_float_data_stays_inside_the_bound_of_two_summation_orders(ctx, float_rirs):
    """|wet - numpy.convolve(x, h)[:n]| <= 2 gamma_T convolve(|x|, |h|)[:n], gamma_T = T u / (1 - T u), u = 2^-53: the bound
    tests/test_gpu_reverb_levels.py derives (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5)"""
    offsets = offsets_of(LENGTHS)
    rng = np.random.default_rng(22)
    speech = speechlike.make(78, LENGTHS[5], "syllables")[0].astype(np.float64)
    wave = np.concatenate([rng.standard_normal(int(offsets[5])) * 3000.0, speech * (1.0 + 2.0 ** -20) + 0.3])
    assert len(wave) == offsets[-1] and not np.array_equal(wave, np.round(wave))
    rirs = [SyntheticRIR(1.0, t, drr_db=-3.0, seed=5, level=l) for l, t in enumerate(TAPS)]
    worst = 0.0
    for room_of in ROOMS:
        got = pick(ctx, wave, offsets, rirs, room_of)
        assert np.isfinite(got).all()
        for b, l in enumerate(room_of):
            x, y = cut(wave, offsets, b), cut(got, offsets, b)
            if l == K:
                assert np.array_equal(bits(y), bits(x))
                continue
            if not len(x):
                continue
            T = len(rirs[l])
            gamma = T * 2.0 ** -53 / (1 - T * 2.0 ** -53)
            err = np.abs(y - reference(x, rirs[l]))
            bound = 2 * gamma * np.convolve(np.abs(x), np.abs(rirs[l]))[:len(x)]
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (room_of, b, float((err / bound).max()))
    print("largest error / bound:", worst)


def test_an_utterances_bytes_depend_on_its_samples_and_its_room_alone(ctx, int_case, float_rirs, float_levels):
    """Alone or in the batch, first or last, whatever rooms the others have - and whatever order the tiles run in: the batches
    below have their costs ascending, descending and wildly unequal (three tiles under one tap beside one tile under 2500), so
    that the cost-sorted tile list is a real permutation of the natural one, and option reverb_pick_sort = 0 runs the natural one."""
    wave, offsets, _ = int_case
    want = lambda b, l: float_levels[l, int(offsets[b]):int(offsets[b + 1])]
    for b in range(1, B):                                                             # alone
        x = np.ascontiguousarray(cut(wave, offsets, b))
        for l in range(K + 1):
            assert np.array_equal(bits(pick(ctx, x, offsets_of((len(x),)), float_rirs, (l,))), bits(want(b, l))), (b, l)
    orders = [(5, 4, 3, 2, 1, 0), (1, 2, 4, 5, 3, 0), (5, 1, 4, 0, 2, 3)]
    rooms = [(0, 2, 3, 1, 2, 2),          # the three-tile utterance under one tap first, 2500 taps on single tiles behind it
             (2, 2, 2, 2, 2, 2),          # costs ascending with the tile's place, and all rooms equal
             (0, 0, 1, 2, 1, 3), (3, 3, 3, 0, 3, 1)]
    for order in orders:
        flat = np.concatenate([cut(wave, offsets, b) for b in order])
        off = offsets_of([LENGTHS[b] for b in order])
        for room_of in rooms:
            for sort in (1, 0):
                with ctx.options(reverb_pick_sort=sort):
                    got = pick(ctx, flat, off, float_rirs, room_of)
                for i, (b, l) in enumerate(zip(order, room_of)):
                    assert np.array_equal(bits(cut(got, off, i)), bits(want(b, l))), (order, room_of, sort, i)


def test_dry_batches_convert_exactly_and_calls_repeat(ctx, int_case, float_rirs):
    wave, offsets, _ = int_case
    dry = wave.astype(np.float64)
    assert np.array_equal(bits(pick(ctx, wave, offsets, float_rirs, None)), bits(dry))              # room_of == NULL
    assert np.array_equal(bits(pick(ctx, wave, offsets, [], (0,) * B)), bits(dry))                    # K == 0
    assert np.array_equal(bits(pick(ctx, wave, offsets, [], None, DEV)), bits(dry))                   # ... and rir == NULL
    as_f64 = dry * 0.37
    assert np.array_equal(bits(pick(ctx, as_f64, offsets, float_rirs, (K,) * B)), bits(as_f64))       # every room the dry one
    a = pick(ctx, wave, offsets, float_rirs, ROOMS[1])
    assert np.array_equal(bits(a), bits(pick(ctx, wave, offsets, float_rirs, ROOMS[1])))              # a second call


def test_empty_batches(ctx):
    out = np.empty(4)
    bits(out)[...] = FILL
    h, ro, room = np.array([1.0, 0.5]), np.array([0, 2], np.int64), np.zeros(2, np.int32)
    assert raw_pick(ctx, None, I16, np.zeros(1, np.int64), 0, h, ro, 1, None, None) == _lib.F2_OK
    assert raw_pick(ctx, None, I16, np.zeros(3, np.int64), 2, h, ro, 1, room, out) == _lib.F2_OK
    assert raw_pick(ctx, None, F64, np.zeros(3, np.int64), 2, None, None, 0, None, out, DEV) == _lib.F2_OK
    assert (bits(out) == FILL).all()


CASES = ["K<0", "rir NULL", "room 3", "room -1", "K=65", "rir_offsets NULL", "rir_offsets[0]=1", "rir_offsets decreasing", "no taps",
         "tap nan", "tap inf", "32769 taps", "B<0", "wave_dtype", "offsets NULL", "offsets[0]=1", "offsets decreasing", "wave NULL",
         "wet NULL", "mem_space"]


@pytest.mark.parametrize("case", CASES)
def test_bad_arguments_leave_the_output_alone(ctx, case):
    lengths = (65, 2, 63)
    offsets = offsets_of(lengths)
    wave = np.arange(int(offsets[-1])).astype(np.int16)
    rir, ro, k = np.array([1.0, 0.5, 0.25, 1.0]), np.array([0, 3, 4], np.int64), 2
    room = np.array([0, 2, 1], np.int32)
    nb, dtype, mem, want, word = 3, I16, HOST, _lib.F2_ERR_INVALID, None
    out = np.empty(len(wave))
    bits(out)[...] = FILL
    dst = out
    if case == "K<0":
        k, word = -1, "K=-1"
    elif case == "rir NULL":
        rir, word = None, "rir is NULL"
    elif case.startswith("room "):
        room[1], word = int(case.split()[1]), "utterance 1"
    elif case == "K=65":
        rir, ro, k, want = np.ones(65), np.arange(66, dtype=np.int64), 65, _lib.F2_ERR_UNSUPPORTED
    elif case == "rir_offsets NULL":
        ro = None
    elif case == "rir_offsets[0]=1":
        ro = np.array([1, 3, 4], np.int64)
    elif case == "rir_offsets decreasing":
        ro = np.array([0, 3, 2], np.int64)
    elif case == "no taps":
        ro = np.array([0, 4, 4], np.int64)
    elif case.startswith("tap "):
        rir[3] = np.nan if case == "tap nan" else -np.inf
    elif case == "32769 taps":
        rir, ro, want = np.full(32770, 1e-3), np.array([0, 1, 32770], np.int64), _lib.F2_ERR_UNSUPPORTED
    elif case == "B<0":
        nb = -1
    elif case == "wave_dtype":
        dtype = 2
    elif case == "offsets NULL":
        offsets = None
    elif case == "offsets[0]=1":
        offsets = offsets.copy()
        offsets[0] = 1
    elif case == "offsets decreasing":
        offsets = offsets.copy()
        offsets[2] = offsets[1] - 1
    elif case == "wave NULL":
        wave = None
    elif case == "wet NULL":
        dst = None
    else:
        mem = 7
    assert raw_pick(ctx, wave, dtype, offsets, nb, rir, ro, k, room, dst, mem) == want, case
    if word:
        assert word in ctx.lib.f2_last_error(ctx.handle).decode(), case
    assert (bits(out) == FILL).all(), case
