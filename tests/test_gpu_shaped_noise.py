"""f2_shaped_noise_levels / f2_eval_shaped_noise_sweep: a ragged batch under K coloured noises and clean in one device pass. The
noise is held against a NumPy restatement of the header's formula (Philox4x32-10 -> two 53-bit uniforms -> Box-Muller cosine branch
-> the level's FIR filter over deviates whose index wraps below zero), the one-tap filter [1.0] - on raw bytes - against the white
sweep, the evaluation - on raw bits - against f2_eval_batch_strided(F2_WAVE_F64) on the waveforms the call returns, and the tally
against counts made from the returned labels. All through the C ABI via ctypes, as tests/test_gpu_noise_sweep.py."""
import os

import numpy as np
import pytest

import f2cnn_oracle as orc
import speechlike
from devmem import Arena
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

C, RADIUS, STEP = 128, 5, 160
R = 2 * RADIUS + 1
# empty, a single sample, both sides of a tile edge (1024 outputs per workgroup), one window (n = 11 * step + 1), a few thousand
LENGTHS = (0, 1, 1023, 1024, 1025, 1761, 4000)
B = len(LENGTHS)
SNR = (10.0, -3.0, 20.0)
K = len(SNR)
U = (K + 1) * B
SEED = 0x1234_5678_9ABC
FILL = 0x5A
TAPS = {"short": (1, 5, 1024), "long": (2, 1025, 2048)}      # the filters of the two K = 3 calls

# ---- the generator of include/f2cnn_hip.h (f2_eval_noise_sweep), restated ---------------------------------------------------
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two; -> four uint64 arrays holding the 32-bit output words"""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2        # 32 x 32 -> 64 bit: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def deviates_at(seed, level, utt, i):
    """z of the samples whose 64-bit indices are the uint64 array i, of utterance `utt` at level `level`"""
    i = np.asarray(i, dtype=np.uint64)
    w0, w1, w2, w3 = philox4x32_10((i & MASK, i >> np.uint64(32), level, utt), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((w0 >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (w1 >> np.uint64(6)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = ((w2 >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (w3 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def wrapped_indices(T, n):
    """(i - t) mod 2^64 for every i < n, t < T that the formula reads: -(T - 1) .. n - 1 as uint64"""
    return np.arange(-(T - 1), n, dtype=np.int64).astype(np.uint64)


def test_restatement_gives_the_published_known_answers_and_wraps():
    """Random123's kat_vectors for philox4x32-10; the samples before the utterance have the counter words (low, 0xffffffff, l, b)"""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = " ".join("{:08x}".format(int(w)) for w in philox4x32_10(counter, key))
        assert got == want, (counter, key)
    i = wrapped_indices(3, 2)
    assert [int(v) for v in i] == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]
    assert [int(v) for v in i >> np.uint64(32)] == [0xffffffff, 0xffffffff, 0, 0]
    z = deviates_at(SEED, 0, 1, wrapped_indices(2048, 2000))
    assert np.isfinite(z).all() and np.abs(z).max() < 8.6 and abs(z.mean()) < 0.1 and abs(z.std() - 1) < 0.1


def formula(clean, s, h, seed, l, b):
    """(want, bound) of the header's formula for one utterance at one level: want = clean + s * c, c the filtered deviates;
    |got - want| <= 2^-52 |want| + s * (1e-13 sum|h| + 2 T 2^-53 sum_t |h[t]| |z[i-t]|)"""
    n, T = len(clean), len(h)
    if n == 0:
        return np.zeros(0), np.zeros(0)
    z = deviates_at(seed, l, b, wrapped_indices(T, n))
    c = np.convolve(z, h)[T - 1:T - 1 + n]                       # c[i] = sum_t h[t] z[i - t]
    mag = np.convolve(np.abs(z), np.abs(h))[T - 1:T - 1 + n]
    want = clean + s * c
    return want, 2.0 ** -52 * np.abs(want) + s * (1e-13 * np.abs(h).sum() + 2 * T * 2.0 ** -53 * mag)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))


@pytest.fixture(scope="module")
def model():
    return F2CNNModel(orc.glorot_weights(7))


def ragged_waves(lengths, seed=40):
    waves = []
    for i, n in enumerate(lengths):
        waves.append(speechlike.make(seed + i, n, "syllables")[0] if n == 4000 else orc.synth_utterance(seed + i, n))
    offsets = np.zeros(len(lengths) + 1, np.int64)
    offsets[1:] = np.cumsum(lengths)
    return np.concatenate(waves).astype(np.int16), offsets


@pytest.fixture(scope="module")
def batch():
    return ragged_waves(LENGTHS)


def random_filter(taps, seed):
    """seeded random taps, normalised to sum h^2 = 1; not symmetric"""
    h = np.random.default_rng([seed, taps]).standard_normal(taps)
    return h / np.sqrt(np.dot(h, h))


def filters_of(taps):
    return [np.ones(1) if t == 1 else random_filter(t, 5) for t in taps]


def pack(firs):
    return _lib._pack_rirs(firs)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def tiled_offsets(offsets, levels):
    total = int(offsets[-1])
    return np.concatenate([[0]] + [l * total + offsets[1:] for l in range(levels)]).astype(np.int64)


def n_windows(lengths, hop, levels):
    return levels * sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in lengths)


class Out:
    """every output of one call, pre-filled with 0x5A"""
    NAMES = ("noisy", "scores", "labels", "wo", "sigma", "stats")

    def __init__(self, offsets, hop, levels=K + 1):
        lengths, nb = np.diff(offsets), len(offsets) - 1
        self.noisy = filled(levels * int(offsets[-1]), np.float64)
        self.scores = filled((n_windows(lengths, hop, levels), 2), np.float32)
        self.labels = filled(n_windows(lengths, hop, levels), np.uint8)
        self.wo = filled(levels * nb + 1, np.int64)
        self.sigma = filled(levels * nb, np.float64)
        self.stats = filled((levels * nb, 2), np.int64)

    def untouched(self):
        return all((bits(getattr(self, name)) == FILL).all() for name in self.NAMES)


p = lambda a: None if a is None else a.ctypes.data


def raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, snr, fir, fo, k, seed, o, lpf=False):
    return ctx.lib.f2_eval_shaped_noise_sweep(ctx.handle, model.handle(ctx), p(wave), dtype, p(offsets), p(coefs), len(offsets) - 1, C,
                                              int(lpf), 50.0 if lpf else 0.0, _lib.FFT_F32, RADIUS, STEP, hop, p(snr), p(fir), p(fo), k,
                                              seed, p(o.noisy), p(o.scores), p(o.labels), p(o.wo), p(o.sigma), p(o.stats), _lib.MEM_HOST)


def sweep(ctx, model, coefs, wave, dtype, offsets, hop, firs, snr=SNR, seed=SEED, lpf=False):
    fir, fo = pack(firs)
    o = Out(offsets, hop, len(firs) + 1)
    rc = raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, np.array(snr, np.float64), fir, fo, len(firs), seed, o, lpf=lpf)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return o


def raw_levels(ctx, wave, dtype, offsets, snr, fir, fo, k, seed, noisy, sigma):
    return ctx.lib.f2_shaped_noise_levels(ctx.handle, p(wave), dtype, p(offsets), len(offsets) - 1, p(snr), p(fir), p(fo), k, seed,
                                          p(noisy), p(sigma), _lib.MEM_HOST)


def levels(ctx, wave, dtype, offsets, firs, snr=SNR, seed=SEED):
    """the stateless entry -> (noisy, sigma)"""
    fir, fo = pack(firs)
    k, nb = len(firs), len(offsets) - 1
    noisy, sigma = filled((k + 1) * int(offsets[-1]), np.float64), filled((k + 1) * nb, np.float64)
    rc = raw_levels(ctx, wave, dtype, offsets, np.array(snr, np.float64), fir, fo, k, seed, noisy, sigma)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return noisy, sigma


@pytest.fixture(scope="module")
def frame_sweeps(ctx, model, coefs, batch):
    """the int16 batch at hop 160 through both sets of filters: shared by the tests that only read it"""
    flat, offsets = batch
    return {name: sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, filters_of(taps)) for name, taps in TAPS.items()}


def white_sweep(ctx, model, coefs, wave, dtype, offsets, hop, o, mem_space=_lib.MEM_HOST, ptrs=None):
    snr = np.array(SNR)
    a = ptrs or dict(wave=p(wave), noisy=p(o.noisy), scores=p(o.scores), labels=p(o.labels))
    rc = ctx.lib.f2_eval_noise_sweep(ctx.handle, model.handle(ctx), a["wave"], dtype, p(offsets), p(coefs), len(offsets) - 1, C, 0, 0.0,
                                     _lib.FFT_F32, RADIUS, STEP, hop, p(snr), K, SEED, a["noisy"], a["scores"], a["labels"], p(o.wo),
                                     p(o.sigma), p(o.stats), mem_space)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return o


# ---- 1. identity with the white sweep -----------------------------------------------------------------------------------------
def test_one_tap_filters_are_the_white_sweep_in_host_memory(ctx, model, coefs, batch):
    flat, offsets = batch
    got = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, [np.ones(1)] * K)
    want = white_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, Out(offsets, 160))
    assert want.wo[-1] > 0
    for name in Out.NAMES:
        assert np.array_equal(bits(getattr(got, name)), bits(getattr(want, name))), name


def device_sweep(ctx, model, coefs, flat, offsets, hop, firs, white=False, misalign=(0, 0, 0, 0), check=False):
    """either sweep with wave, noisy, scores and labels in an arena of device memory"""
    o = Out(offsets, hop, len(firs) + 1)
    with Arena(ctx) as arena:
        arena.region("wave", np.int16, len(flat), misalign=misalign[0], role="in")
        arena.region("noisy", np.float64, o.noisy.size, misalign=misalign[1], role="out")
        arena.region("scores", np.float32, o.scores.size, misalign=misalign[2], role="out")
        arena.region("labels", np.uint8, o.labels.size, misalign=misalign[3], role="out")
        arena.upload("wave", flat)
        ptrs = {name: arena.ptr(name) for name in ("wave", "noisy", "scores", "labels")}
        if white:
            white_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, o, _lib.MEM_DEVICE, ptrs)
        else:
            fir, fo = pack(firs)
            snr = np.array(SNR)
            rc = ctx.lib.f2_eval_shaped_noise_sweep(ctx.handle, model.handle(ctx), ptrs["wave"], _lib.WAVE_I16, p(offsets), p(coefs), B, C,
                                                    0, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, p(snr), p(fir), p(fo), len(firs), SEED,
                                                    ptrs["noisy"], ptrs["scores"], ptrs["labels"], p(o.wo), p(o.sigma), p(o.stats),
                                                    _lib.MEM_DEVICE)
            assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        ctx.synchronize()
        if check:
            arena.check()
            assert arena.unwritten("noisy") == 0 and arena.unwritten("scores") == 0
        o.noisy[...] = arena.download("noisy")
        o.scores[...] = arena.download("scores").reshape(o.scores.shape)
        o.labels[...] = arena.download("labels")
    return o


def test_one_tap_filters_are_the_white_sweep_in_device_memory(ctx, model, coefs, batch):
    flat, offsets = batch
    got = device_sweep(ctx, model, coefs, flat, offsets, 160, [np.ones(1)] * K)
    want = device_sweep(ctx, model, coefs, flat, offsets, 160, [np.ones(1)] * K, white=True)
    for name in Out.NAMES:
        assert np.array_equal(bits(getattr(got, name)), bits(getattr(want, name))), name


# ---- 2. the header's formula --------------------------------------------------------------------------------------------------
def check_formula(noisy, sigma, flat, offsets, firs, seed=SEED, stream=None):
    """every (level, utterance) of a call against formula(); -> the worst error / bound"""
    k, nb, total = len(firs), len(offsets) - 1, int(offsets[-1])
    noisy = noisy.reshape(k + 1, total)
    assert np.array_equal(noisy[k], flat.astype(np.float64))                     # the clean level, exactly
    assert (sigma[k * nb:] == 0).all()
    worst = 0.0
    for l in range(k):
        for b in range(nb):
            clean = flat[offsets[b]:offsets[b + 1]].astype(np.float64)
            want, bound = formula(clean, sigma[l * nb + b], firs[l], seed, l if stream is None else stream[l], b)
            err = np.abs(noisy[l, offsets[b]:offsets[b + 1]] - want)
            if len(clean):
                worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (l, b, float((err / bound).max()))
    return worst


def numpy_sigma(flat, offsets, snr):
    nb = len(offsets) - 1
    want = np.zeros((len(snr) + 1) * nb)
    for l, v in enumerate(snr):
        for b in range(nb):
            w = flat[offsets[b]:offsets[b + 1]]
            if len(w):
                want[l * nb + b] = np.sqrt(np.mean(np.square(w.astype(np.float64)))) / 10 ** (v / 10)
    return want


@pytest.mark.parametrize("name", list(TAPS))
def test_noise_is_the_headers_formula(batch, frame_sweeps, name):
    flat, offsets = batch
    o = frame_sweeps[name]
    want = numpy_sigma(flat, offsets, SNR)
    assert (np.abs(o.sigma - want) <= np.spacing(want)).all()
    worst = check_formula(o.noisy, o.sigma, flat, offsets, filters_of(TAPS[name]))
    print("taps", TAPS[name], "worst error / bound", worst)


@pytest.mark.parametrize("n", [1, 3, 1025])
def test_every_tap_count_up_to_sixteen_is_the_headers_formula(ctx, n):
    """sixteen levels of 1 .. 16 taps: every combination of the walk's paired turns (0 .. 2), its single step (0 / 1) and its 0 .. 3
    last taps; 1025 samples have a full tile and a tile of one output, 1 and 3 samples a lane with fewer outputs than it owns (the
    samples are not zero, so that no sigma is and every level is filtered noise)"""
    flat = np.random.default_rng([70, n]).integers(1000, 20000, n).astype(np.int16)
    offsets = np.array([0, n], np.int64)
    firs = [random_filter(t, 7) for t in range(1, 17)]
    noisy, sigma = levels(ctx, flat, _lib.WAVE_I16, offsets, firs, snr=(3.0,) * 16)
    assert (sigma[:16] > 0).all()
    worst = check_formula(noisy, sigma, flat, offsets, firs)
    print("n", n, "worst error / bound", worst)


def test_a_span_that_crosses_two_tiles_and_wraps_below_zero(ctx):
    """2048 taps on 2500 samples: the span of the second tile starts inside the first, the first one's 2047 samples below zero"""
    flat, offsets = ragged_waves((2500,), seed=60)
    firs = [random_filter(2048, 6)]
    for dtype, wave in ((_lib.WAVE_I16, flat), (_lib.WAVE_F64, flat.astype(np.float64))):
        noisy, sigma = levels(ctx, wave, dtype, offsets, firs, snr=(3.0,))
        worst = check_formula(noisy, sigma, flat, offsets, firs)
        print("dtype", dtype, "worst error / bound", worst)


def test_the_bound_tells_a_shifted_and_a_reversed_filter_apart(ctx, batch):
    flat, offsets = batch
    h = np.array([0.7, -0.5, 0.4, 0.25, -0.2])
    h /= np.sqrt(np.dot(h, h))
    noisy, sigma = levels(ctx, flat, _lib.WAVE_I16, offsets, [h], snr=(0.0,))
    check_formula(noisy, sigma, flat, offsets, [h])
    lo, hi, b = offsets[6], offsets[7], 6                                        # the 4000-sample utterance
    clean = flat[lo:hi].astype(np.float64)
    for other in (np.roll(h, 1), h[::-1].copy(), np.concatenate([[0.0], h[:-1]])):
        want, bound = formula(clean, sigma[b], other, SEED, 0, b)
        ratio = np.abs(noisy[lo:hi] - want) / bound
        print("wrong filter: worst error / bound", float(ratio.max()), "violations", int((ratio > 1).sum()))
        assert (ratio > 1).sum() > 3900                                          # nearly every sample, not a stray one


# ---- 3. independence ----------------------------------------------------------------------------------------------------------
def alone(flat, offsets, b):
    """utterance b at position b of a batch of empty neighbours"""
    solo = np.zeros(B + 1, np.int64)
    solo[b + 1:] = offsets[b + 1] - offsets[b]
    return flat[offsets[b]:offsets[b + 1]].copy(), solo


@pytest.mark.parametrize("name", list(TAPS))
def test_an_utterance_does_not_depend_on_its_neighbours(ctx, batch, frame_sweeps, name):
    flat, offsets = batch
    total = int(offsets[-1])
    full = frame_sweeps[name].noisy.reshape(K + 1, total)
    for b in range(1, B):
        wave, solo = alone(flat, offsets, b)
        noisy, sigma = levels(ctx, wave, _lib.WAVE_I16, solo, filters_of(TAPS[name]))
        assert np.array_equal(bits(noisy.reshape(K + 1, -1)), bits(full[:, offsets[b]:offsets[b + 1]])), b
        assert np.array_equal(bits(sigma.reshape(K + 1, B)[:, b]), bits(frame_sweeps[name].sigma.reshape(K + 1, B)[:, b])), b


def test_the_sweep_of_an_utterance_alone(ctx, model, coefs, batch, frame_sweeps):
    """(the entry points take no utterance number: an utterance keeps its number by keeping its place, among empty neighbours)"""
    flat, offsets = batch
    b, total = 5, int(offsets[-1])
    wave, solo = alone(flat, offsets, b)
    o = sweep(ctx, model, coefs, wave, _lib.WAVE_I16, solo, 160, filters_of(TAPS["long"]))
    full = frame_sweeps["long"]
    assert np.array_equal(bits(o.noisy.reshape(K + 1, -1)), bits(full.noisy.reshape(K + 1, total)[:, offsets[b]:offsets[b + 1]]))
    rows = [l * B + b for l in range(K + 1)]
    assert np.array_equal(o.stats[rows], full.stats[rows]) and np.array_equal(bits(o.sigma[rows]), bits(full.sigma[rows]))
    assert np.array_equal(bits(o.scores), bits(np.concatenate([full.scores[full.wo[u]:full.wo[u + 1]] for u in rows])))


def test_permuted_levels_move_the_filter_and_the_snr_not_the_stream(ctx, batch, frame_sweeps):
    flat, offsets = batch
    firs, perm = filters_of(TAPS["short"]), (2, 0, 1)
    noisy, sigma = levels(ctx, flat, _lib.WAVE_I16, offsets, [firs[j] for j in perm], snr=[SNR[j] for j in perm])
    base = frame_sweeps["short"]
    for l, j in enumerate(perm):
        assert np.array_equal(bits(sigma[l * B:(l + 1) * B]), bits(base.sigma[j * B:(j + 1) * B]))
    check_formula(noisy, sigma, flat, offsets, [firs[j] for j in perm])                  # level l draws stream l
    total = int(offsets[-1])
    assert not np.array_equal(noisy[:total], base.noisy[2 * total:3 * total])             # not the old level's samples


def test_int16_and_float64_input_of_equal_values_give_the_same_bytes(ctx, batch, frame_sweeps):
    """(the sums of squares of these int16 values stay below 2^53, so the float64 sum is exact too and sigma is the same)"""
    flat, offsets = batch
    for name, taps in TAPS.items():
        noisy, sigma = levels(ctx, flat.astype(np.float64), _lib.WAVE_F64, offsets, filters_of(taps))
        assert np.array_equal(bits(noisy), bits(frame_sweeps[name].noisy)), name
        assert np.array_equal(bits(sigma), bits(frame_sweeps[name].sigma)), name


def test_two_seeds_differ(ctx, batch, frame_sweeps):
    flat, offsets = batch
    total = int(offsets[-1])
    noisy, sigma = levels(ctx, flat, _lib.WAVE_I16, offsets, filters_of(TAPS["short"]), seed=SEED + 1)
    base = frame_sweeps["short"]
    assert not np.array_equal(bits(noisy[:K * total]), bits(base.noisy[:K * total]))
    assert np.array_equal(bits(noisy[K * total:]), bits(base.noisy[K * total:])) and np.array_equal(bits(sigma), bits(base.sigma))
    check_formula(noisy, sigma, flat, offsets, filters_of(TAPS["short"]), seed=SEED + 1)


# ---- 4. the stateless entry against the sweep ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TAPS))
def test_stateless_entry_returns_the_sweeps_bytes(ctx, batch, frame_sweeps, name):
    flat, offsets = batch
    noisy, sigma = levels(ctx, flat, _lib.WAVE_I16, offsets, filters_of(TAPS[name]))
    assert np.array_equal(bits(noisy), bits(frame_sweeps[name].noisy))
    assert np.array_equal(bits(sigma), bits(frame_sweeps[name].sigma))


# ---- 5. evaluation: no tolerance ----------------------------------------------------------------------------------------------
def numpy_stats(labels, wo, k, nb):
    want = np.zeros(((k + 1) * nb, 2), np.int64)
    for u in range((k + 1) * nb):
        mine = labels[wo[u]:wo[u + 1]]
        clean = labels[wo[k * nb + u % nb]:wo[k * nb + u % nb + 1]]
        want[u] = mine.sum(), (mine == clean).sum()
    return want


@pytest.mark.parametrize("hop", (1, 160))
def test_evaluation_is_the_strided_call_on_the_returned_waveforms(ctx, model, coefs, batch, frame_sweeps, hop):
    flat, offsets = batch
    o = frame_sweeps["long"] if hop == 160 else sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, filters_of(TAPS["long"]))
    nw = n_windows(LENGTHS, hop, K + 1)
    sc, lb = filled((nw, 2), np.float32), filled(nw, np.uint8)
    wo = ctx.eval_batch_strided(model.handle(ctx), o.noisy, _lib.WAVE_F64, tiled_offsets(offsets, K + 1), coefs, U, C, False, 0.0,
                                _lib.FFT_F32, RADIUS, STEP, hop, sc, lb, _lib.MEM_HOST)
    assert np.array_equal(o.wo, wo) and o.wo[-1] == nw > 0
    assert np.array_equal(bits(o.scores), bits(sc))
    assert np.array_equal(o.labels, lb) and set(np.unique(o.labels)) <= {0, 1}
    assert np.array_equal(o.stats, numpy_stats(o.labels, o.wo, K, B))
    windows = np.diff(o.wo)
    assert np.array_equal(o.stats[K * B:, 1], windows[K * B:])                   # the clean level agrees with itself


# ---- 6. placement ---------------------------------------------------------------------------------------------------------------
def test_sweep_buffers_at_odd_misalignments_between_guard_bands(ctx, model, coefs, batch, frame_sweeps):
    flat, offsets = batch
    o = device_sweep(ctx, model, coefs, flat, offsets, 160, filters_of(TAPS["long"]), misalign=(1, 3, 1, 3), check=True)
    for name in Out.NAMES:
        assert np.array_equal(bits(getattr(o, name)), bits(getattr(frame_sweeps["long"], name))), name


def test_stateless_buffers_at_odd_misalignments_between_guard_bands(ctx, batch, frame_sweeps):
    flat, offsets = batch
    firs = filters_of(TAPS["long"])
    fir, fo = pack(firs)
    snr, sigma = np.array(SNR), filled(U, np.float64)
    with Arena(ctx) as arena:
        arena.region("wave", np.int16, len(flat), misalign=3, role="in")
        arena.region("noisy", np.float64, (K + 1) * len(flat), misalign=5, role="out")
        arena.upload("wave", flat)
        rc = ctx.lib.f2_shaped_noise_levels(ctx.handle, arena.ptr("wave"), _lib.WAVE_I16, p(offsets), B, p(snr), p(fir), p(fo), K, SEED,
                                            arena.ptr("noisy"), p(sigma), _lib.MEM_DEVICE)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        ctx.synchronize()
        arena.check()
        assert arena.unwritten("noisy") == 0
        noisy = arena.download("noisy")
    assert np.array_equal(bits(noisy), bits(frame_sweeps["long"].noisy)) and np.array_equal(bits(sigma), bits(frame_sweeps["long"].sigma))


# ---- 7. call history ------------------------------------------------------------------------------------------------------------
def test_the_sweep_does_not_depend_on_what_the_context_ran_before(coefs, batch, frame_sweeps):
    flat, offsets = batch
    other, other_offsets = ragged_waves((3000, 1900), seed=70)
    used, fresh = _lib.Context(0), _lib.Context(0)
    try:
        m = F2CNNModel(orc.glorot_weights(7))
        white_sweep(used, m, coefs, other, _lib.WAVE_I16, other_offsets, 7, Out(other_offsets, 7))
        used.eval_reverb_sweep(m.handle(used), other, _lib.WAVE_I16, other_offsets, coefs, 2, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, 160,
                               [random_filter(300, 1), random_filter(1500, 2)], None, None, None, _lib.MEM_HOST)
        sweep(used, m, coefs, other.astype(np.float64), _lib.WAVE_F64, other_offsets, 7, [random_filter(77, 3)], snr=(5.0,), seed=3)
        a = sweep(used, m, coefs, flat, _lib.WAVE_I16, offsets, 160, filters_of(TAPS["long"]))
        b = sweep(fresh, m, coefs, flat, _lib.WAVE_I16, offsets, 160, filters_of(TAPS["long"]))
    finally:
        used.close()
        fresh.close()
    for name in Out.NAMES:
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(frame_sweeps["long"], name))), name


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
ERROR_CASES = {
    # name: (status, the words of the message that name the level, or None)
    "K=0": (INVALID, None), "snr NULL": (INVALID, None), "snr nan": (INVALID, None), "offsets decreasing": (INVALID, None),
    "fir NULL": (INVALID, None), "fir_offsets NULL": (INVALID, None), "fir_offsets[0] != 0": (INVALID, "level 0"),
    "fir_offsets decreasing": (INVALID, "level 1"), "a level with no taps": (INVALID, "level 2"),
    "a tap that is not finite": (INVALID, "level 1"), "too many taps": (UNSUPPORTED, "level 1"), "K=65": (UNSUPPORTED, None),
}


def error_arguments(case, batch):
    flat, offsets = batch
    firs = [np.ones(1), np.ones(3) / np.sqrt(3), np.ones(2) / np.sqrt(2)]
    snr, k = np.array(SNR), K
    fir, fo = pack(firs)
    if case == "K=0":
        k = 0
    elif case == "snr NULL":
        snr = None
    elif case == "snr nan":
        snr = np.array([10.0, np.nan, 3.0])
    elif case == "offsets decreasing":
        offsets = offsets.copy()
        offsets[3] = offsets[2] - 1
    elif case == "fir NULL":
        fir = None
    elif case == "fir_offsets NULL":
        fo = None
    elif case == "fir_offsets[0] != 0":
        fo = fo + 1
        fir = np.concatenate([[0.5], fir])
    elif case == "fir_offsets decreasing":
        fo = np.array([0, 4, 3, 6], np.int64)
    elif case == "a level with no taps":
        fo = np.array([0, 1, 6, 6], np.int64)
    elif case == "a tap that is not finite":
        fir = fir.copy()
        fir[2] = np.inf
    elif case == "too many taps":
        fir, fo = pack([np.ones(1), np.ones(2049) / np.sqrt(2049), np.ones(2)])
    elif case == "K=65":
        k, snr = 65, np.zeros(65)
        fir, fo = pack([np.ones(1)] * 65)
    return flat, offsets, snr, fir, fo, k


@pytest.mark.parametrize("case", list(ERROR_CASES) + ["hop=0"])
def test_bad_arguments_of_the_sweep_leave_the_outputs_alone(ctx, model, coefs, batch, case):
    status, word = ERROR_CASES.get(case, (INVALID, None))
    flat, offsets, snr, fir, fo, k = error_arguments(case, batch)
    o = Out(batch[1], 160)
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 0 if case == "hop=0" else 160, snr, fir, fo, k, SEED, o)
    message = ctx.lib.f2_last_error(ctx.handle).decode()
    print(case, "->", rc, message)
    assert rc == status, case
    assert o.untouched(), case
    assert word is None or word in message, message


@pytest.mark.parametrize("case", list(ERROR_CASES))
def test_bad_arguments_of_the_stateless_entry_leave_the_outputs_alone(ctx, batch, case):
    status, word = ERROR_CASES[case]
    flat, offsets, snr, fir, fo, k = error_arguments(case, batch)
    noisy, sigma = filled((K + 1) * len(flat), np.float64), filled(U, np.float64)
    rc = raw_levels(ctx, flat, _lib.WAVE_I16, offsets, snr, fir, fo, k, SEED, noisy, sigma)
    message = ctx.lib.f2_last_error(ctx.handle).decode()
    assert rc == status, case
    assert (bits(noisy) == FILL).all() and (bits(sigma) == FILL).all(), case
    assert word is None or word in message, message


def test_no_window_anywhere_still_fills_the_small_outputs(ctx, model, coefs):
    """as the white sweep fills them: window offsets and stats zero, sigma of the samples that are there"""
    flat, offsets = ragged_waves((1700, 0), seed=50)
    firs = filters_of(TAPS["short"])
    o = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, firs)
    assert (o.wo == 0).all() and (o.stats == 0).all()
    rms = np.sqrt(np.mean(np.square(flat.astype(np.float64))))
    assert np.allclose(o.sigma, [rms / 10, 0, rms / 10 ** -0.3, 0, rms / 100, 0, 0, 0], rtol=1e-15)
    check_formula(o.noisy, o.sigma, flat, offsets, firs)
    none = np.zeros(3, np.int64)                                                  # two utterances, no sample
    o = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, none, 160, firs)
    assert (o.wo == 0).all() and (o.stats == 0).all() and (o.sigma == 0).all()
    noisy, sigma = levels(ctx, flat, _lib.WAVE_I16, none, firs)
    assert (sigma == 0).all()
    empty = Out(np.zeros(1, np.int64), 160)
    fir, fo = pack(firs)
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, np.zeros(1, np.int64), 160, np.array(SNR), fir, fo, K, SEED, empty)
    assert rc == _lib.F2_OK and empty.wo[0] == 0
    assert raw_levels(ctx, flat, _lib.WAVE_I16, np.zeros(1, np.int64), np.array(SNR), fir, fo, K, SEED, None, None) == _lib.F2_OK


# ---- 9. the command line, end to end ------------------------------------------------------------------------------------------
def test_cli_writes_a_reproducible_coloursweep_and_leaves_the_white_sweep_alone(tmp_path, monkeypatch, capsys, coefs):
    from scipy.io import wavfile
    from f2cnn_amd import cli, config, noise
    monkeypatch.chdir(tmp_path)
    config.write_default()
    m = F2CNNModel(orc.glorot_weights(7))
    m.save("model.npz")
    wave = orc.synth_utterance(77, 5000).astype(np.int16)
    wav = str(tmp_path / "DR1.FAAA0.SA1.WAV")
    wavfile.write(wav, 16000, wave)
    rng = np.random.default_rng(8)
    wavfile.write("babble.wav", 16000, (np.convolve(rng.standard_normal(6000), noise.ColourFIR("pink", 16000, 129), "same") * 3000)
                  .astype(np.int16))
    np.save("taps.npy", np.array([1.0, -0.9]))
    argv = ["cnn", "noisesweep", "--file", wav, "--snrs", "10,-3", "--seed", "11", "--hop", "frame", "--model", "model.npz"]
    colours = ["--colours", "white,speech,like:babble.wav,fir:taps.npy", "--noise-taps", "129"]
    assert cli.main(argv + colours) == 0
    out = os.path.join("OutputWavFiles", "addedNoise", "DR1.FAAA0.SA1.coloursweep.npz")
    first = dict(np.load(out))
    kk = 8
    assert sorted(first) == sorted(["snr_db", "colours", "sigma", "windows", "rising", "agree", "agreement", "seed", "hop", "fir",
                                    "fir_offsets", "labels_clean"] + ["labels_%d" % k for k in range(kk)])
    n = len(range(0, 5000 - R * STEP, STEP))
    assert first["windows"].tolist() == [n] * (kk + 1) and int(first["hop"]) == STEP and int(first["seed"]) == 11
    assert first["snr_db"].tolist() == [10.0, -3.0] * 4
    assert first["colours"].tolist() == ["white"] * 2 + ["speech"] * 2 + ["babble"] * 2 + ["taps"] * 2
    assert first["fir_offsets"].tolist() == [0, 1, 2, 131, 260, 389, 518, 520, 522] and len(first["fir"]) == 522
    assert np.array_equal(first["fir"][2:131], noise.ColourFIR("speech", 16000, 129))
    assert np.allclose(first["fir"][518:520], np.array([1.0, -0.9]) / np.sqrt(1.81), rtol=1e-15)
    assert first["sigma"][kk] == 0 and (first["sigma"][:kk] > 0).all()
    for k in range(kk):
        assert first["labels_%d" % k].shape == (n,) and first["rising"][k] == first["labels_%d" % k].sum()
        assert first["agree"][k] == (first["labels_%d" % k] == first["labels_clean"]).sum()
    printed = capsys.readouterr().out
    assert "speech 10dB" in printed and "babble -3dB" in printed and "taps 10dB" in printed and "clean" in printed
    assert not os.path.exists(os.path.join("OutputWavFiles", "addedNoise", "DR1.FAAA0.SA1.sweep.npz"))
    assert cli.main(argv + colours) == 0
    second = dict(np.load(out))
    for key in first:
        assert np.array_equal(bits(first[key]), bits(second[key])), key
    # without the option: the white sweep, held against a direct call of its entry point
    assert cli.main(argv) == 0
    white = dict(np.load(os.path.join("OutputWavFiles", "addedNoise", "DR1.FAAA0.SA1.sweep.npz")))
    assert sorted(white) == sorted(["snr_db", "sigma", "windows", "rising", "agree", "agreement", "seed", "hop", "labels_0", "labels_1",
                                    "labels_clean"])
    ctx = _lib.default_context()
    offsets = np.array([0, 5000], np.int64)
    labels = np.empty(3 * n, np.uint8)
    wo, sigma, stats = ctx.eval_noise_sweep(m.handle(ctx), wave, _lib.WAVE_I16, offsets, coefs, 1, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP,
                                            STEP, [10.0, -3.0], 11, None, None, labels, _lib.MEM_HOST)
    assert np.array_equal(bits(white["sigma"]), bits(sigma)) and np.array_equal(white["rising"], stats[:, 0])
    for k, key in enumerate(("labels_0", "labels_1", "labels_clean")):
        assert np.array_equal(white[key], labels[wo[k]:wo[k + 1]])
    # the white colour's levels have the white sweep's indices, so they are its levels
    assert np.array_equal(bits(first["sigma"][:2]), bits(sigma[:2]))
    assert np.array_equal(first["labels_0"], white["labels_0"]) and np.array_equal(first["labels_1"], white["labels_1"])
