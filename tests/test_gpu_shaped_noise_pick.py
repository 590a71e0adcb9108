"""f2_shaped_noise_pick: a ragged batch under coloured noise with one level (filter, SNR) per utterance, in the layout of the waves.
Held on raw bytes against the level it picks of f2_shaped_noise_levels (the sweep makes every level; the pick must be its level
level_of[b] of utterance b), against f2_noise_pick with one-tap filters of 1.0, and within the sweep test's own bound against the
NumPy restatement of the header's formula with utterance number first_utterance + b (tests/test_gpu_shaped_noise.py: philox4x32_10,
deviates_at, formula - imported, the bound not widened). All through the C ABI via ctypes."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib
from f2cnn_amd.reverb import SyntheticRIR
from test_gpu_shaped_noise import bits, deviates_at, filled, formula, pack, philox4x32_10, random_filter  # noqa: F401 (the generator)

pytestmark = pytest.mark.gpu

# empty, a single sample, both sides of a tile edge (1024 outputs per workgroup), three tiles with a short last one
LENGTHS = (0, 1, 1023, 1024, 1025, 3000)
B = len(LENGTHS)
TAPS = (1, 5, 1025, 2048)             # one tap, a tail that is no multiple of four, both sides of the odd designs, the most
SNR = (10.0, -3.0, 20.0, 3.0)
K = len(SNR)
FIRS = [random_filter(t, 5) for t in TAPS]
ROTATIONS = [tuple((b + r) % (K + 1) for b in range(B)) for r in range(K + 1)]      # every (utterance, level) pair once
SEED = 0x1234_5678_9ABC
FILL = 0x5A
DTYPE = {_lib.WAVE_I16: np.int16, _lib.WAVE_F64: np.float64}
p = lambda a: None if a is None else a.ctypes.data


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def waves(dt, lengths=LENGTHS, seed=40):
    flat = np.concatenate([orc.synth_utterance(seed + i, n) for i, n in enumerate(lengths)] + [np.zeros(0)]).astype(np.int16)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return (flat if dt == _lib.WAVE_I16 else flat.astype(np.float64) * 0.37), offsets


def pick(ctx, flat, dt, offsets, firs, level_of, first=0, snr=SNR, seed=SEED, mem=_lib.MEM_HOST):
    """-> (noisy, sigma), both pre-filled"""
    nb = len(offsets) - 1
    noisy, sigma = filled(len(flat), np.float64), filled(nb, np.float64)
    if mem == _lib.MEM_HOST:
        ctx.shaped_noise_pick(flat, dt, offsets, nb, snr, firs, level_of, first, seed, noisy, mem, sigma=sigma)
        return noisy, sigma
    d_in, d_out = ctx.malloc(max(flat.nbytes, 8)), ctx.malloc(max(noisy.nbytes, 8))
    try:
        ctx.h2d(d_in, flat)
        ctx.h2d(d_out, noisy)
        ctx.synchronize()
        ctx.shaped_noise_pick(d_in, dt, offsets, nb, snr, firs, level_of, first, seed, d_out, mem, sigma=sigma)
        ctx.synchronize()
        ctx.d2h(noisy, d_out)
        ctx.synchronize()
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    return noisy, sigma


def sweep_levels(ctx, flat, dt, offsets, firs, snr=SNR, seed=SEED):
    """f2_shaped_noise_levels -> (noisy (K+1, total), sigma (K+1, B))"""
    nb, k = len(offsets) - 1, len(firs)
    noisy = filled((k + 1) * len(flat), np.float64)
    sigma = ctx.shaped_noise_levels(flat, dt, offsets, nb, snr, firs, seed, noisy, _lib.MEM_HOST)
    return noisy.reshape(k + 1, len(flat)), sigma.reshape(k + 1, nb)


def picked(sweep, offsets, level_of):
    """what the pick must return: utterance b from level level_of[b] of the sweep"""
    noisy, sigma = sweep
    out = np.empty(noisy.shape[1])
    for b, l in enumerate(level_of):
        out[offsets[b]:offsets[b + 1]] = noisy[l, offsets[b]:offsets[b + 1]]
    return out, np.array([sigma[l, b] for b, l in enumerate(level_of)])


@pytest.fixture(scope="module")
def sweeps(ctx):
    """the sweep of the batch, once per dtype; read only"""
    out = {}
    for dt in DTYPE:
        flat, offsets = waves(dt)
        out[dt] = sweep_levels(ctx, flat, dt, offsets, FIRS)
        for a in out[dt]:
            a.setflags(write=False)
    return out


# ---- 1. identity with the sweep -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", (_lib.MEM_HOST, _lib.MEM_DEVICE))
@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_every_utterance_is_its_level_of_the_sweep(ctx, sweeps, dt, mem):
    flat, offsets = waves(dt)
    for level_of in ROTATIONS:
        noisy, sigma = pick(ctx, flat, dt, offsets, FIRS, level_of, mem=mem)
        want, want_sigma = picked(sweeps[dt], offsets, level_of)
        assert bits(noisy).tobytes() == bits(want).tobytes(), level_of
        assert bits(sigma).tobytes() == bits(want_sigma).tobytes(), level_of
    # the noise is there, and the clean level is the samples themselves
    noisy, sigma = pick(ctx, flat, dt, offsets, FIRS, ROTATIONS[0], mem=mem)
    assert ROTATIONS[0][4] == K and np.array_equal(noisy[offsets[4]:offsets[5]], flat[offsets[4]:offsets[5]].astype(np.float64))
    assert sigma[4] == 0 and sigma[3] > 0 and not np.array_equal(noisy[offsets[3]:offsets[4]], flat[offsets[3]:offsets[4]])


# ---- 2. the header's formula, utterance number first_utterance + b ---------------------------------------------------------------
@pytest.mark.parametrize("first", (0, 7, 2 ** 32 - B))
def test_formula_with_the_utterance_number_of_the_corpus(ctx, first):
    flat, offsets = waves(_lib.WAVE_F64)
    worst = 0.0
    for level_of in ROTATIONS:
        noisy, sigma = pick(ctx, flat, _lib.WAVE_F64, offsets, FIRS, level_of, first=first)
        for b, l in enumerate(level_of):
            clean, got = flat[offsets[b]:offsets[b + 1]], noisy[offsets[b]:offsets[b + 1]]
            if l == K or len(clean) == 0:
                assert sigma[b] == 0 and np.array_equal(got, clean), (b, l)
                continue
            assert np.isclose(sigma[b], np.sqrt(np.mean(clean * clean)) / 10 ** (SNR[l] / 10), rtol=1e-12), (b, l)
            want, bound = formula(clean, sigma[b], FIRS[l], SEED, l, first + b)
            err = np.abs(got - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (first, b, l, float((err / bound).max()))
    print("first_utterance {}: worst error / bound = {:.3g}".format(first, worst))
    if first:      # ... and it is not the noise of utterance number b
        other, _ = pick(ctx, flat, _lib.WAVE_F64, offsets, FIRS, ROTATIONS[0], first=0)
        noisy, _ = pick(ctx, flat, _lib.WAVE_F64, offsets, FIRS, ROTATIONS[0], first=first)
        assert not np.array_equal(other[offsets[5]:], noisy[offsets[5]:])


# ---- 3. identity with white ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
@pytest.mark.parametrize("first", (0, 5))
def test_one_tap_filters_of_one_are_noise_pick(ctx, dt, first):
    flat, offsets = waves(dt)
    for level_of in ROTATIONS[1:3]:
        noisy, sigma = pick(ctx, flat, dt, offsets, [np.ones(1)] * K, level_of, first=first)
        want = filled(len(flat), np.float64)
        want_sigma = ctx.noise_pick(flat, dt, offsets, B, SNR, level_of, first, SEED, want, _lib.MEM_HOST, sigma=True)
        assert bits(noisy).tobytes() == bits(want).tobytes() and bits(sigma).tobytes() == bits(want_sigma).tobytes(), level_of


# ---- 4. every tap count up to 16; the longest filter across a tile edge --------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3, 1025))
def test_every_tap_count_up_to_sixteen(ctx, n):
    firs = [random_filter(t, 8) for t in range(1, 17)]
    snr = tuple(float(3 * (l % 5)) for l in range(16))
    flat, offsets = waves(_lib.WAVE_F64, (n,) * 17, seed=70)
    level_of = tuple(range(17))                             # level b for utterance b, the last one clean
    noisy, sigma = pick(ctx, flat, _lib.WAVE_F64, offsets, firs, level_of, snr=snr)
    want, want_sigma = picked(sweep_levels(ctx, flat, _lib.WAVE_F64, offsets, firs, snr=snr), offsets, level_of)
    assert bits(noisy).tobytes() == bits(want).tobytes() and bits(sigma).tobytes() == bits(want_sigma).tobytes()
    worst = 0.0
    for b in range(16):
        clean, got = flat[offsets[b]:offsets[b + 1]], noisy[offsets[b]:offsets[b + 1]]
        f, bound = formula(clean, sigma[b], firs[b], SEED, b, b)
        worst = max(worst, float((np.abs(got - f) / bound).max()))
        assert (np.abs(got - f) <= bound).all(), (b, worst)
    print("n = {}: worst error / bound = {:.3g}".format(n, worst))
    assert np.array_equal(noisy[offsets[16]:], flat[offsets[16]:])


def test_the_span_of_the_second_tile_starts_inside_the_first_and_wraps(ctx):
    """2048 taps on 2500 samples: output 1024 reads deviates -1023 .. 1024, and output 0 reads -2047 .. 0"""
    flat, offsets = waves(_lib.WAVE_F64, (2500,), seed=90)
    h = [random_filter(2048, 9)]
    noisy, sigma = pick(ctx, flat, _lib.WAVE_F64, offsets, h, (0,), snr=(6.0,))
    want, want_sigma = picked(sweep_levels(ctx, flat, _lib.WAVE_F64, offsets, h, snr=(6.0,)), offsets, (0,))
    assert bits(noisy).tobytes() == bits(want).tobytes() and bits(sigma).tobytes() == bits(want_sigma).tobytes()
    f, bound = formula(flat, sigma[0], h[0], SEED, 0, 0)
    print("2048 taps on 2500 samples: worst error / bound = {:.3g}".format(float((np.abs(noisy - f) / bound).max())))
    assert (np.abs(noisy - f) <= bound).all()


# ---- 5. independence ----------------------------------------------------------------------------------------------------------------
def test_a_sample_depends_on_its_own_utterance_level_and_number_alone(ctx):
    flat, offsets = waves(_lib.WAVE_I16)
    level_of = ROTATIONS[2]                                     # (2, 3, 4, 0, 1, 2)
    ref, ref_sigma = pick(ctx, flat, _lib.WAVE_I16, offsets, FIRS, level_of)
    # a repeated call
    again, _ = pick(ctx, flat, _lib.WAVE_I16, offsets, FIRS, level_of)
    assert bits(again).tobytes() == bits(ref).tobytes()
    for b in range(B):
        own = slice(int(offsets[b]), int(offsets[b + 1]))
        # alone, as utterance number b of its corpus
        alone, s = pick(ctx, np.ascontiguousarray(flat[own]), _lib.WAVE_I16, np.array([0, LENGTHS[b]], np.int64), FIRS, (level_of[b],), first=b)
        assert bits(alone).tobytes() == bits(ref[own]).tobytes() and bits(s).tobytes() == bits(ref_sigma[b:b + 1]).tobytes(), b
        # the others at other levels
        others = tuple(l if u == b else (l + 1 + u % 3) % (K + 1) for u, l in enumerate(level_of))
        assert others[b] == level_of[b] and all(o != l for u, (o, l) in enumerate(zip(others, level_of)) if u != b)
        moved, _ = pick(ctx, flat, _lib.WAVE_I16, offsets, FIRS, others)
        assert bits(moved[own]).tobytes() == bits(ref[own]).tobytes(), b
    # the tile list utterance by utterance
    with ctx.options(noise_pick_sort=0):
        unsorted, s = pick(ctx, flat, _lib.WAVE_I16, offsets, FIRS, level_of)
    assert bits(unsorted).tobytes() == bits(ref).tobytes() and bits(s).tobytes() == bits(ref_sigma).tobytes()
    assert ctx.get_option("noise_pick_sort") == 1


def test_a_context_that_ran_other_stages_first_gives_the_same_bytes(ctx):
    flat, offsets = waves(_lib.WAVE_I16)
    level_of = ROTATIONS[3]
    ref, ref_sigma = pick(ctx, flat, _lib.WAVE_I16, offsets, FIRS, level_of)
    other = _lib.Context(0)
    try:
        big, big_off = waves(_lib.WAVE_F64, (5000, 300), seed=12)
        scratch = np.empty(len(big))
        other.noise_pick(big, _lib.WAVE_F64, big_off, 2, (0.0,), (0, 1), 3, 99, scratch, _lib.MEM_HOST)
        sweep_levels(other, big, _lib.WAVE_F64, big_off, [random_filter(77, 1), random_filter(2048, 2)], snr=(1.0, 2.0), seed=3)
        other.reverb_pick(big, _lib.WAVE_F64, big_off, 2, [SyntheticRIR(1.0, 3000, seed=2, level=0)], (0, 1), scratch, _lib.MEM_HOST)
        got, sigma = pick(other, flat, _lib.WAVE_I16, offsets, FIRS, level_of)
    finally:
        other.close()
    assert bits(got).tobytes() == bits(ref).tobytes() and bits(sigma).tobytes() == bits(ref_sigma).tobytes()


# ---- 6. clean, zero and empty -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_clean_calls_convert_exactly_without_taps(ctx, dt):
    flat, offsets = waves(dt)
    want = flat.astype(np.float64)
    for snr, level_of in (((), None), ((), (0,) * B), (SNR, None), (SNR, (K,) * B)):
        noisy, sigma = pick(ctx, flat, dt, offsets, None, level_of, snr=snr)
        assert bits(noisy).tobytes() == bits(want).tobytes() and not sigma.any(), (snr, level_of)
    # ... and with taps that are not looked at
    noisy, sigma = pick(ctx, flat, dt, offsets, FIRS, (K,) * B)
    assert bits(noisy).tobytes() == bits(want).tobytes() and not sigma.any()


def test_an_all_zero_utterance_at_a_noisy_level_is_copied(ctx):
    flat, offsets = waves(_lib.WAVE_F64, (1500, 700), seed=21)
    flat[:1500] = 0.0
    noisy, sigma = pick(ctx, flat, _lib.WAVE_F64, offsets, FIRS, (2, 2))
    assert sigma[0] == 0 and sigma[1] > 0
    assert bits(noisy[:1500]).tobytes() == bits(np.zeros(1500)).tobytes() and not np.array_equal(noisy[1500:], flat[1500:])


def test_an_empty_batch_is_ok(ctx):
    fir, fo = pack(FIRS)
    snr, off0 = np.array(SNR), np.zeros(1, np.int64)
    sigma = filled(2, np.float64)
    call = ctx.lib.f2_shaped_noise_pick
    assert call(ctx.handle, None, _lib.WAVE_I16, None, 0, p(snr), p(fir), p(fo), K, None, 0, SEED, None, None, _lib.MEM_HOST) == _lib.F2_OK
    assert call(ctx.handle, None, _lib.WAVE_I16, p(off0), 0, p(snr), p(fir), p(fo), K, None, 0, SEED, None, None, _lib.MEM_DEVICE) == _lib.F2_OK
    # utterances without samples: sigma comes back as zeros
    lev, off = np.array([0, 1], np.int32), np.zeros(3, np.int64)
    assert call(ctx.handle, None, _lib.WAVE_F64, p(off), 2, p(snr), p(fir), p(fo), K, p(lev), 0, SEED, None, p(sigma), _lib.MEM_HOST) == _lib.F2_OK
    assert not sigma.any()


# ---- 7. errors, before anything is launched or written ------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(ctx):
    flat, offsets = waves(_lib.WAVE_I16)
    fir, fo = pack(FIRS)
    base = dict(wave=flat, dt=_lib.WAVE_I16, offsets=offsets, nb=B, snr=np.array(SNR), fir=fir, fo=fo, k=K,
                level=np.array(ROTATIONS[1], np.int32), first=0, mem=_lib.MEM_HOST)
    noisy, sigma = filled(len(flat), np.float64), filled(B, np.float64)

    def call(**kw):
        a = dict(dict(base, noisy=noisy), **kw)
        return ctx.lib.f2_shaped_noise_pick(ctx.handle, p(a["wave"]), a["dt"], p(a["offsets"]), a["nb"], p(a["snr"]), p(a["fir"]), p(a["fo"]),
                                            a["k"], p(a["level"]), a["first"], SEED, p(a["noisy"]), p(sigma), a["mem"])
    INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    bad_level, nan_snr = base["level"].copy(), base["snr"].copy()
    bad_level[3], nan_snr[1] = K + 1, np.nan
    off1, down = offsets.copy(), offsets.copy()
    off1[0], down[3] = 1, offsets[2] - 1
    nan_tap, fo1, fo_down, fo_empty, fo_long = fir.copy(), fo.copy(), fo.copy(), fo.copy(), fo.copy()
    nan_tap[fo[2] + 7], fo1[0], fo_down[2], fo_empty[2], fo_long[4] = np.inf, 1, fo[1] - 1, fo[1], fo[3] + 2049
    k65 = 65
    cases = [
        # those of f2_noise_pick
        (dict(dt=7), INV, "dtype"), (dict(nb=-1), INV, "B=-1"), (dict(mem=9), INV, "mem"), (dict(k=-1), INV, "K=-1"),
        (dict(level=bad_level), INV, "utterance 3"), (dict(snr=None), INV, "snr_db is NULL"), (dict(snr=nan_snr), INV, "snr_db[1]"),
        (dict(first=2 ** 32 - B + 1), UNS, "32-bit"), (dict(offsets=None), INV, "offsets"), (dict(offsets=off1), INV, "offsets[0]"),
        (dict(offsets=down), INV, "non-decreasing"), (dict(wave=None), INV, "null data"), (dict(noisy=None), INV, "null data"),
        # those of the taps, by f2_shaped_noise_levels' checks
        (dict(fir=None), INV, "fir"), (dict(fo=None), INV, "fir_offsets"),
        (dict(k=k65, snr=np.zeros(k65), fir=np.ones(k65), fo=np.arange(k65 + 1, dtype=np.int64)), UNS, "65"),
        (dict(fir=np.ones(fo_long[4]), fo=fo_long), UNS, "level 3"), (dict(fo=fo_empty), INV, "level 1"),
        (dict(fir=nan_tap), INV, "level 2"), (dict(fo=fo1), INV, "fir_offsets[0]"), (dict(fo=fo_down), INV, "level 1"),
    ]
    for kw, status, word in cases:
        assert call(**kw) == status, (list(kw), ctx.lib.f2_last_error(ctx.handle).decode())
        assert word in ctx.lib.f2_last_error(ctx.handle).decode(), (list(kw), ctx.lib.f2_last_error(ctx.handle).decode())
        assert (bits(noisy) == FILL).all() and (bits(sigma) == FILL).all(), list(kw)
    assert call() == _lib.F2_OK and np.isfinite(noisy).all() and np.isfinite(sigma).all()
