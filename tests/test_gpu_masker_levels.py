"""f2_masker_levels: a ragged batch under K recorded maskers and clean in one device pass, against the NumPy restatement of the
header's contract (tests/masker_cases.py): the start of every segment exactly, sigma on raw bits against f2_eval_noise_sweep, the
gain against a correctly rounded sum within a derived bound, and every sample on raw bits from the returned gain. All through the C
ABI via ctypes, as tests/test_gpu_shaped_noise.py."""
import numpy as np
import pytest

import f2cnn_oracle as orc
import masker_cases as mc
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel
from masker_cases import B, K, LENGTHS, SEED, bits, filled, ptr
from test_gpu_shaped_noise import philox4x32_10

pytestmark = pytest.mark.gpu

U = (K + 1) * B
INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch():
    return mc.ragged_waves()


def raw_levels(ctx, wave, dtype, offsets, snr, masker, moff, r, mof, k, seed, noisy, sigma, gain, start, mem=_lib.MEM_HOST):
    return ctx.lib.f2_masker_levels(ctx.handle, ptr(wave) if isinstance(wave, np.ndarray) else wave, dtype, ptr(offsets), len(offsets) - 1,
                                    ptr(snr), ptr(masker), ptr(moff), r, ptr(mof), k, seed,
                                    ptr(noisy) if isinstance(noisy, np.ndarray) else noisy, ptr(sigma), ptr(gain), ptr(start), mem)


def levels(ctx, wave, dtype, offsets, recordings, masker_of, snr, seed=SEED):
    """the stateless entry on host memory -> (noisy, sigma, gain, start), every output pre-filled"""
    masker, moff = _lib._pack_rirs(recordings)
    k, nb = len(snr), len(offsets) - 1
    u = (k + 1) * nb
    noisy, sigma, gain, start = filled((k + 1) * int(offsets[-1]), np.float64), filled(u, np.float64), filled(u, np.float64), filled(u, np.int64)
    rc = raw_levels(ctx, wave, dtype, offsets, np.array(snr, np.float64), masker, moff, len(recordings), np.array(masker_of, np.int32), k, seed,
                    noisy, sigma, gain, start)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return noisy, sigma, gain, start


@pytest.fixture(scope="module")
def results(ctx, batch):
    """one call per set of recordings, shared (and left unchanged) by the tests below"""
    wave, offsets = batch
    return {name: levels(ctx, wave, _lib.WAVE_I16, offsets, *SET) for name, SET in mc.SETS.items()}


def test_restatement_gives_the_published_known_answers():
    """Random123's kat_vectors for philox4x32-10, and the start is the low 64 bits of the draw modulo the length"""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        assert " ".join("{:08x}".format(int(w)) for w in philox4x32_10(counter, key)) == want, (counter, key)
    w = [int(v) for v in philox4x32_10((3, mc.STREAM, 0, 5), (SEED & 0xFFFFFFFF, SEED >> 32))]
    assert mc.start_of(SEED, 3, 5, 5000) == ((w[1] << 32) | w[0]) % 5000 and mc.start_of(SEED, 3, 5, 1) == 0


@pytest.mark.parametrize("name", list(mc.SETS))
def test_start_is_the_restated_start_and_levels_of_one_recording_share_it(results, name):
    recordings, masker_of, _ = mc.SETS[name]
    start = results[name][3].reshape(K + 1, B)
    for l, r in enumerate(masker_of):
        for b in range(B):
            assert int(start[l, b]) == mc.start_of(SEED, r, b, len(recordings[r])), (l, b)
    assert (start[K] == 0).all()
    twins = [(l, m) for l in range(K) for m in range(l + 1, K) if masker_of[l] == masker_of[m]]
    assert twins and all(np.array_equal(start[l], start[m]) for l, m in twins)


def test_the_seed_shows_both_sides_of_every_edge():
    """the 5000-sample recordings: a segment that wraps and one that does not; the late one: silent segments and others"""
    recordings, masker_of, _ = mc.SETS["wraps"]
    wraps = [mc.start_of(SEED, 3, b, 5000) + n > 5000 for b, n in enumerate(LENGTHS) if n]
    assert any(wraps) and not all(wraps)
    late = mc.SETS["silent"][0][1]
    quiet = [not mc.segment(late, mc.start_of(SEED, 1, b, 5000), n).any() for b, n in enumerate(LENGTHS) if n]
    assert any(quiet) and not all(quiet)
    assert all(mc.start_of(SEED, 1, b, 7) + n > 7 for b, n in enumerate(LENGTHS) if n >= 1023)      # hundreds of wraps


@pytest.mark.parametrize("name", list(mc.SETS))
def test_sigma_is_the_white_sweeps_on_raw_bits(ctx, batch, results, name):
    wave, offsets = batch
    snr = mc.SETS[name][2]
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, mc.C, 100))
    model = F2CNNModel(orc.glorot_weights(7))
    _, white, _ = ctx.eval_noise_sweep(model.handle(ctx), wave, _lib.WAVE_I16, offsets, coefs, B, mc.C, False, 0.0, _lib.FFT_F32, mc.RADIUS,
                                       mc.STEP, mc.STEP, snr, SEED, None, None, None, _lib.MEM_HOST)
    assert bits(results[name][1]).tobytes() == bits(white).tobytes()
    assert (white.reshape(K + 1, B)[:K, 2:] > 0).all() and (white.reshape(K + 1, B)[K] == 0).all()


@pytest.mark.parametrize("name", list(mc.SETS))
def test_gain_within_the_bound_of_the_fixed_order_sum(batch, results, name):
    recordings, masker_of, _ = mc.SETS[name]
    _, sigma, gain, start = (a.reshape(K + 1, B) if a.size == U else a for a in results[name])
    worst = 0.0
    for l, r in enumerate(masker_of):
        for b, n in enumerate(LENGTHS):
            want, rtol = mc.gain_of(float(sigma[l, b]), recordings[r], int(start[l, b]), n)
            if want == 0.0:
                assert gain[l, b] == 0.0 and not np.signbit(gain[l, b]), (l, b)
                continue
            err = abs(gain[l, b] - want) / want
            worst = max(worst, err / rtol)
            print(f"{name} level {l} utterance {b} (n={n}): gain {gain[l, b]!r}, relative error {err:.3e}, bound {rtol:.3e}")
            assert err <= rtol, (l, b)
    assert (gain[K] == 0).all() and np.isfinite(gain).all()
    print(f"{name}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name", list(mc.SETS))
def test_every_sample_is_the_mix_on_raw_bits(batch, results, name):
    wave, offsets = batch
    recordings, masker_of, _ = mc.SETS[name]
    noisy, sigma, gain, start = results[name]
    total = int(offsets[-1])
    noisy, gain, start = noisy.reshape(K + 1, total), gain.reshape(K + 1, B), start.reshape(K + 1, B)
    assert np.isfinite(noisy).all()
    changed = 0
    for l, r in enumerate(masker_of):
        for b in range(B):
            clean = wave[offsets[b]:offsets[b + 1]]
            want = mc.mixed(clean, float(gain[l, b]), recordings[r], int(start[l, b]))
            assert bits(noisy[l, offsets[b]:offsets[b + 1]]).tobytes() == bits(want).tobytes(), (l, b)
            changed += int(gain[l, b] != 0.0)
    assert changed >= B                                     # (the maskers are there)
    # level K, silent segments and empty utterances: the clean values exactly, and gain 0
    assert bits(noisy[K]).tobytes() == bits(wave.astype(np.float64)).tobytes()
    for l, r in enumerate(masker_of):
        for b, n in enumerate(LENGTHS):
            if n == 0 or not mc.segment(recordings[r], int(start[l, b]), n).any():
                assert gain[l, b] == 0.0
                assert bits(noisy[l, offsets[b]:offsets[b + 1]]).tobytes() == bits(wave[offsets[b]:offsets[b + 1]].astype(np.float64)).tobytes()


def test_an_all_zero_utterance_stays_clean(ctx):
    wave = np.concatenate([np.zeros(1025, np.int16), orc.synth_utterance(3, 2000).astype(np.int16)])
    offsets = np.array([0, 1025, 3025], np.int64)
    noisy, sigma, gain, start = levels(ctx, wave, _lib.WAVE_I16, offsets, *mc.SETS["wraps"])
    noisy, gain, sigma = noisy.reshape(K + 1, -1), gain.reshape(K + 1, 2), sigma.reshape(K + 1, 2)
    assert (gain[:, 0] == 0).all() and (sigma[:, 0] == 0).all() and (gain[:K, 1] > 0).all()
    assert (bits(noisy[:, :1025]) == 0).all() and not np.array_equal(noisy[0, 1025:], noisy[K, 1025:])


def test_same_bits_from_float64_input_and_device_memory(ctx, batch, results):
    wave, offsets = batch
    SET = mc.SETS["wraps"]
    want = results["wraps"]
    got = levels(ctx, wave.astype(np.float64), _lib.WAVE_F64, offsets, *SET)
    for g, w in zip(got, want):
        assert bits(g).tobytes() == bits(w).tobytes()
    masker, moff = _lib._pack_rirs(SET[0])
    total = int(offsets[-1])
    out = filled((K + 1) * total, np.float64)
    sigma, gain, start = filled(U, np.float64), filled(U, np.float64), filled(U, np.int64)
    d_in, d_out = ctx.malloc(wave.nbytes), ctx.malloc(out.nbytes)
    try:
        ctx.h2d(d_in, wave)
        ctx.h2d(d_out, out)
        ctx.synchronize()
        rc = raw_levels(ctx, d_in, _lib.WAVE_I16, offsets, np.array(SET[2], np.float64), masker, moff, len(SET[0]), np.array(SET[1], np.int32), K,
                        SEED, d_out, sigma, gain, start, _lib.MEM_DEVICE)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        ctx.synchronize()
        ctx.d2h(out, d_out)
        ctx.synchronize()
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    for g, w in zip((out, sigma, gain, start), want):
        assert bits(g).tobytes() == bits(w).tobytes()


def test_an_utterance_alone_and_a_level_alone_give_the_same_bits(ctx, batch, results):
    """B = 1 of each utterance, its number supplied through the pick; K = 1 of each level against the K = 5 call. (An empty batch
    launches nothing and reports zeros, so the start of the empty utterance is compared inside the batch only.)"""
    wave, offsets = batch
    recordings, masker_of, snr = mc.SETS["wraps"]
    noisy, sigma, gain, start = results["wraps"]
    total = int(offsets[-1])
    noisy = noisy.reshape(K + 1, total)
    for b, n in enumerate(LENGTHS):
        one = wave[offsets[b]:offsets[b + 1]]
        for l in range(K + 1):
            out = filled(n, np.float64)
            small = ctx.masker_pick(one, _lib.WAVE_I16, np.array([0, n]), 1, snr, recordings, masker_of, [l], b, SEED, out, _lib.MEM_HOST,
                                    small=True)
            assert bits(out).tobytes() == bits(noisy[l, offsets[b]:offsets[b + 1]]).tobytes(), (b, l)
            for got, want in zip(small, (sigma, gain, start) if n else ()):
                assert bits(got).tobytes() == bits(want.reshape(K + 1, B)[l, b:b + 1]).tobytes(), (b, l)
    for l in range(K):
        got = levels(ctx, wave, _lib.WAVE_I16, offsets, recordings, masker_of[l:l + 1], snr[l:l + 1])
        assert bits(got[0][:total]).tobytes() == bits(noisy[l]).tobytes(), l
        assert bits(got[0][total:]).tobytes() == bits(noisy[K]).tobytes(), l
        for g, w in zip(got[1:], (sigma, gain, start)):
            assert bits(g[:B]).tobytes() == bits(w.reshape(K + 1, B)[l]).tobytes(), l


def test_an_empty_batch_fills_the_small_outputs_with_zeros(ctx):
    recordings, masker_of, snr = mc.SETS["wraps"]
    noisy, sigma, gain, start = levels(ctx, np.zeros(0, np.int16), _lib.WAVE_I16, np.zeros(3, np.int64), recordings, masker_of, snr)
    assert len(noisy) == 0 and (sigma == 0).all() and (gain == 0).all() and (start == 0).all() and len(start) == 2 * (K + 1)


def test_every_error_comes_before_anything_is_written(ctx, batch):
    wave, offsets = batch
    recordings, masker_of, snr = mc.SETS["wraps"]
    masker, moff = _lib._pack_rirs(recordings)
    total = int(offsets[-1])
    outs = [filled((K + 1) * total, np.float64), filled(U, np.float64), filled(U, np.float64), filled(U, np.int64)]

    def call(snr=np.array(snr, np.float64), masker=masker, moff=moff, r=len(recordings), mof=np.array(masker_of, np.int32), k=K, offsets=offsets,
             dtype=_lib.WAVE_I16):
        return raw_levels(ctx, wave, dtype, offsets, snr, masker, moff, r, mof, k, SEED, *outs)
    nan_snr, nan_masker, inf_masker = np.array(snr, np.float64), masker.copy(), masker.copy()
    nan_snr[2], nan_masker[1 + 7 + 3], inf_masker[0] = np.nan, np.nan, np.inf
    late, falling, empty, bad_of, neg_of = moff.copy(), moff.copy(), moff.copy(), np.array(masker_of, np.int32), np.array(masker_of, np.int32)
    late[0], falling[2], empty[2], bad_of[4], neg_of[0] = 1, 0, empty[1], 4, -1
    long_off = np.array([0, (1 << 26) + 1], np.int64)
    many = np.arange(66, dtype=np.int64)
    bad_offsets = offsets.copy()
    bad_offsets[3] = bad_offsets[2] - 1
    cases = (
        (dict(masker=None), INV, "masker"), (dict(moff=None), INV, "masker_offsets"), (dict(mof=None), INV, "masker_of"),
        (dict(moff=late), INV, "masker_offsets[0]"), (dict(moff=falling), INV, "recording 1"), (dict(moff=empty), INV, "recording 1 is empty"),
        (dict(masker=nan_masker), INV, "recording 2: sample 3"), (dict(masker=inf_masker), INV, "recording 0: sample 0"),
        (dict(mof=bad_of), INV, "level 4"), (dict(mof=neg_of), INV, "level 0"), (dict(r=0), INV, "R=0"),
        (dict(k=0), INV, "K=0"), (dict(snr=None), INV, "snr_db"), (dict(snr=nan_snr), INV, "snr_db[2]"),
        (dict(moff=many, r=65, masker=np.ones(65)), UNS, "65 recordings"),
        (dict(k=65, snr=np.zeros(65), mof=np.zeros(65, np.int32)), UNS, "65 masker levels"),
        (dict(moff=long_off, r=1, mof=np.zeros(K, np.int32)), UNS, "recording 0 has 67108865 samples"),
        (dict(offsets=bad_offsets), INV, "offsets"), (dict(dtype=7), INV, "wave_dtype"),
    )
    for kw, status, word in cases:
        assert call(**kw) == status, list(kw)
        msg = ctx.lib.f2_last_error(ctx.handle).decode()
        assert word in msg, (list(kw), msg)
        assert all((bits(o) == mc.FILL).all() for o in outs), list(kw)
    assert call() == _lib.F2_OK and np.isfinite(outs[0]).all()
