"""f2_reverb_levels: a ragged batch convolved with K impulse responses, and dry, in one device pass. Sizes around the two tile
constants of k_reverb_levels (an output tile that ends one sample into the next, a tap chunk boundary on each side, responses
longer than an utterance, the empty utterance), held against numpy.convolve(x, h)[:n]
 - bit for bit where every partial sum is an integer below 2^53 (int16 samples, integer taps),
 - within the textbook bound for two differently ordered float64 dot products elsewhere,
and against themselves on raw bits (a second call, alone / in the batch, K = 1 / K = 6, host / device memory, int16 / float64).
Through the C ABI via ctypes, as tests/test_gpu_noise_sweep.py."""
import numpy as np
import pytest

import speechlike
from f2cnn_amd import _lib
from f2cnn_amd.reverb import SyntheticRIR

pytestmark = pytest.mark.gpu

BLK, TC = _lib.REVERB_BLOCK, _lib.REVERB_TAP_CHUNK
LENGTHS = (0, 1, BLK + 1, 2 * BLK + 37)
TAPS = (1, 2, TC - 1, TC, TC + 1, 3 * TC + 5)
B, K = len(LENGTHS), len(TAPS)
FILL = 0x5A
I16, F64 = _lib.WAVE_I16, _lib.WAVE_F64


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
    return np.concatenate(rirs).astype(np.float64), offsets_of([len(h) for h in rirs])


def raw_levels(ctx, wave, dtype, offsets, nb, rir, rir_offsets, k, levels, mem_space=_lib.MEM_HOST):
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
    return ctx.lib.f2_reverb_levels(ctx.handle, p(wave), dtype, p(offsets), nb, p(rir), p(rir_offsets), k, p(levels), mem_space)


def levels_of(ctx, wave, offsets, rirs):
    """(K + 1, total) float64 of a host-memory call, pre-filled so that an element left out shows"""
    rir, ro = pack(rirs)
    out = np.empty((len(rirs) + 1, int(offsets[-1])), np.float64)
    bits(out)[...] = FILL
    dtype = I16 if wave.dtype == np.int16 else F64
    rc = raw_levels(ctx, wave, dtype, offsets, len(offsets) - 1, rir, ro, len(rirs), out)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return out


def reference(x, h):
    return np.convolve(x.astype(np.float64), h)[:len(x)] if len(x) else np.zeros(0)


@pytest.fixture(scope="module")
def int_case():
    """int16 samples over the full range (the extremes included) and integer taps in [-8, 8]: every product and every partial
    sum is an integer of magnitude below 6e8 < 2^53 (checked here), so any summation order gives the same float64"""
    rng = np.random.default_rng(11)
    offsets = offsets_of(LENGTHS)
    wave = rng.integers(-32768, 32768, int(offsets[-1])).astype(np.int16)
    wave[int(offsets[2]):int(offsets[2]) + 2] = (-32768, 32767)
    rirs = [rng.integers(-8, 9, t).astype(np.float64) for t in TAPS]
    for h in rirs:
        h[0] = h[0] or 1.0
    for b in range(B):
        x = np.abs(wave[offsets[b]:offsets[b + 1]].astype(np.float64))
        if len(x):
            assert max(np.convolve(x, np.abs(h))[:len(x)].max() for h in rirs) < 6e8
    wave.setflags(write=False)
    return wave, offsets, rirs


@pytest.fixture(scope="module")
def int_levels(ctx, int_case):
    out = levels_of(ctx, *int_case)
    out.setflags(write=False)
    return out


def test_integer_data_is_numpys_convolution_bit_for_bit(int_case, int_levels):
    wave, offsets, rirs = int_case
    for l, h in enumerate(rirs):
        for b in range(B):
            x = wave[offsets[b]:offsets[b + 1]]
            got = int_levels[l, offsets[b]:offsets[b + 1]]
            # (an exact integer sum has one float64 but for a zero's sign, which a sum's first term chooses: the accumulator
            # starts from +0 and so never holds -0; + 0.0 takes numpy's zeros there too)
            assert np.array_equal(bits(got), bits(reference(x, h) + 0.0)), (l, b)
    assert np.array_equal(bits(int_levels[K]), bits(wave.astype(np.float64)))        # the dry level


@pytest.mark.parametrize("n", [1, 3, BLK + 1])
def test_every_tap_count_up_to_sixteen_is_numpys_convolution_bit_for_bit(ctx, n):
    """1 .. 16 taps are every combination of the walk's paired turns (0 .. 2), its single step (0 / 1) and its 0 .. 3 last taps; an
    utterance of BLK + 1 samples has a full tile and a tile of one output, those of 1 and 3 samples a lane with fewer outputs than
    it owns. Integer data as in int_case: sums below 16 * 8 * 32768 < 2^53"""
    rng = np.random.default_rng([14, n])
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    rirs = [rng.integers(-8, 9, t).astype(np.float64) for t in range(1, 17)]
    got = levels_of(ctx, x, offsets_of((n,)), rirs)
    for h, y in zip(rirs, got):
        assert np.array_equal(bits(y), bits(reference(x, h) + 0.0)), (n, len(h))
    assert np.array_equal(bits(got[16]), bits(x.astype(np.float64)))


@pytest.mark.parametrize("kind", ["unit", "delay", "half"])
def test_the_three_responses_anyone_can_check_by_eye(ctx, int_case, kind):
    wave, offsets, _ = int_case
    dry = wave.astype(np.float64)
    if kind == "unit":
        got = levels_of(ctx, wave, offsets, [np.array([1.0])])
        assert np.array_equal(bits(got[0]), bits(dry)) and np.array_equal(bits(got[1]), bits(dry))
        return
    if kind == "half":
        got = levels_of(ctx, wave, offsets, [np.array([0.5])])
        assert np.array_equal(got[0], 0.5 * dry)
        return
    for d in (1, TC - 1, TC, BLK + 3):                       # inside a chunk, on its edge, beyond an output tile
        h = np.zeros(d + 1)
        h[d] = 1.0
        got = levels_of(ctx, wave, offsets, [h])[0]
        for b in range(B):
            x, y = dry[offsets[b]:offsets[b + 1]], got[offsets[b]:offsets[b + 1]]
            want = np.concatenate([np.zeros(min(d, len(x))), x[:max(len(x) - d, 0)]])
            assert np.array_equal(y, want), (d, b)


def test_float_data_stays_inside_the_bound_of_two_summation_orders(ctx):
    """|levels - numpy.convolve(x, h)[:n]| <= 2 gamma_T convolve(|x|, |h|)[:n], gamma_T = T u / (1 - T u), u = 2^-53: each of
    the two sums of T products is within gamma_T sum |h x| of the exact value in any order (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., eq. 3.5)"""
    offsets = offsets_of(LENGTHS)
    rng = np.random.default_rng(12)
    speech = speechlike.make(77, LENGTHS[3], "syllables")[0].astype(np.float64)
    wave = np.concatenate([rng.standard_normal(LENGTHS[1] + LENGTHS[2]) * 3000.0, speech * (1.0 + 2.0 ** -20) + 0.3])
    assert len(wave) == offsets[-1] and not np.array_equal(wave, np.round(wave))
    rirs = [SyntheticRIR(1.0, t, drr_db=-3.0, seed=5, level=l) for l, t in enumerate(TAPS)]     # t60 * framerate = t taps
    assert [len(h) for h in rirs] == list(TAPS)
    got = levels_of(ctx, wave, offsets, rirs)
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got[K]), bits(wave))
    worst = 0.0
    for l, h in enumerate(rirs):
        T = len(h)
        gamma = T * 2.0 ** -53 / (1 - T * 2.0 ** -53)
        for b in range(B):
            x = wave[offsets[b]:offsets[b + 1]]
            if not len(x):
                continue
            err = np.abs(got[l, offsets[b]:offsets[b + 1]] - reference(x, h))
            bound = 2 * gamma * np.convolve(np.abs(x), np.abs(h))[:len(x)]
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (l, b, float((err / bound).max()))
    print("largest error / bound:", worst)


def test_a_samples_bits_depend_on_its_utterance_its_response_and_its_index_alone(ctx, int_case):
    wave, offsets, _ = int_case
    # float taps, so that a changed order would show; the samples stay the int16 ones
    rirs = [SyntheticRIR(1.0, t, seed=3, level=l) for l, t in enumerate(TAPS)]
    full = levels_of(ctx, wave, offsets, rirs)
    assert np.array_equal(bits(full), bits(levels_of(ctx, wave, offsets, rirs)))              # a second call
    for b in (1, 2, 3):                                                                        # alone in the batch
        x = np.ascontiguousarray(wave[offsets[b]:offsets[b + 1]])
        alone = levels_of(ctx, x, offsets_of((len(x),)), rirs)
        assert np.array_equal(bits(alone), bits(full[:, offsets[b]:offsets[b + 1]])), b
    for l, h in enumerate(rirs):                                                               # K = 1, and another place in rir
        one = levels_of(ctx, wave, offsets, [h])
        assert np.array_equal(bits(one[0]), bits(full[l])), l
    as_f64 = levels_of(ctx, wave.astype(np.float64), offsets, rirs)                            # the same values as float64
    assert np.array_equal(bits(as_f64), bits(full))
    # device memory
    rir, ro = pack(rirs)
    d_wave, d_out = ctx.malloc(wave.nbytes), ctx.malloc(full.nbytes)
    try:
        ctx.h2d(d_wave, wave)
        ctx.memset(d_out, FILL, full.nbytes)
        assert raw_levels(ctx, d_wave, I16, offsets, B, rir, ro, K, d_out, _lib.MEM_DEVICE) == _lib.F2_OK
        ctx.synchronize()
        dev = np.empty_like(full)
        ctx.d2h(dev, d_out)
    finally:
        ctx.free(d_wave)
        ctx.free(d_out)
    assert np.array_equal(bits(dev), bits(full))


def test_empty_batches(ctx):
    out = np.empty(4)
    bits(out)[...] = FILL
    h, ro = np.array([1.0, 0.5]), np.array([0, 2], np.int64)
    assert raw_levels(ctx, None, I16, np.zeros(1, np.int64), 0, h, ro, 1, None) == _lib.F2_OK
    assert raw_levels(ctx, None, I16, np.zeros(3, np.int64), 2, h, ro, 1, out) == _lib.F2_OK
    assert (bits(out) == FILL).all()


CASES = ["K=0", "K=65", "rir NULL", "rir_offsets NULL", "rir_offsets[0]=1", "rir_offsets decreasing", "no taps", "tap nan", "tap inf",
         "32769 taps", "levels x utterances", "B<0", "wave_dtype", "offsets NULL", "offsets[0]=1", "offsets decreasing", "wave NULL",
         "levels NULL", "mem_space"]


@pytest.mark.parametrize("case", CASES)
def test_bad_arguments_leave_the_output_alone(ctx, case):
    lengths = (65, 2, 63)
    offsets = offsets_of(lengths)
    wave = np.arange(int(offsets[-1])).astype(np.int16)
    rir, ro, k = np.array([1.0, 0.5, 0.25, 1.0]), np.array([0, 3, 4], np.int64), 2
    nb, dtype, mem, want = 3, I16, _lib.MEM_HOST, _lib.F2_ERR_INVALID
    out = np.empty((3, len(wave)))
    bits(out)[...] = FILL
    dst = out
    if case == "K=0":
        k = 0
    elif case == "K=65":
        rir, ro, k, want = np.ones(65), np.arange(66, dtype=np.int64), 65, _lib.F2_ERR_UNSUPPORTED
    elif case == "rir NULL":
        rir = None
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
    elif case == "levels x utterances":
        # 65 levels of 2^24 (empty) utterances: more than f2_eval_noise_sweep's (K+1) * B <= INT32_MAX / 2
        nb = 1 << 24
        offsets, rir, ro, k, want = np.zeros(nb + 1, np.int64), np.ones(64), np.arange(65, dtype=np.int64), 64, _lib.F2_ERR_UNSUPPORTED
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
    elif case == "levels NULL":
        dst = None
    else:
        mem = 7
    assert raw_levels(ctx, wave, dtype, offsets, nb, rir, ro, k, dst, mem) == want, case
    assert (bits(out) == FILL).all(), case


def test_the_longest_response_is_accepted(ctx):
    """32768 taps against an utterance shorter than the response: every chunk beyond the utterance is skipped"""
    rng = np.random.default_rng(13)
    x = rng.integers(-32768, 32768, TC + 3).astype(np.int16)
    h = rng.integers(-8, 9, 32768).astype(np.float64)
    got = levels_of(ctx, x, offsets_of((len(x),)), [h])
    assert np.array_equal(got[0], reference(x, h)) and np.array_equal(bits(got[1]), bits(x.astype(np.float64)))
