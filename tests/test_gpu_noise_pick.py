"""f2_noise_pick: f2_eval_noise_sweep's noise with one level per utterance. Every utterance and its sigma are held bit for bit
against that call's noisy_or_null / sigma_or_null for the same snr_db and seed; then the utterance number, the clean cases,
repeatability and the argument errors. Shapes: tests/noisy_batch.py."""
import numpy as np
import pytest

import noisy_batch as nb
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel
from noisy_batch import B, C, K, LEVEL_OF, LENGTHS, RADIUS, SEED, SNR, STEP, bits, filled, ptr

pytestmark = pytest.mark.gpu

DTYPES = (_lib.WAVE_I16, _lib.WAVE_F64)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sweeps(ctx):
    """per dtype: (flat, offsets, the sweep's noisy levels (K + 1, total), its sigma (K + 1, B)), computed once"""
    model = F2CNNModel.glorot(7, nb.R, C)
    coefs = nb.coefs()
    out = {}
    for dt in DTYPES:
        flat, offsets = nb.waves(dt)
        total = int(offsets[-1])
        noisy = np.empty((K + 1) * total)
        _, sigma, _ = ctx.eval_noise_sweep(model.handle(ctx), flat, dt, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, STEP,
                                           SNR, SEED, noisy, None, None, _lib.MEM_HOST)
        out[dt] = flat, offsets, noisy.reshape(K + 1, total), sigma.reshape(K + 1, B)
    model.release(ctx)
    return out


def pick(ctx, flat, dt, offsets, snr, level_of, first, seed, mem=_lib.MEM_HOST, want_sigma=True, nbatch=None):
    nbatch = len(offsets) - 1 if nbatch is None else nbatch
    total = int(offsets[-1])
    sigma = filled(nbatch, np.float64) if want_sigma else None
    if mem == _lib.MEM_HOST:
        noisy = filled(total, np.float64)
        ctx.noise_pick(flat, dt, offsets, nbatch, snr, level_of, first, seed, noisy, mem, sigma=sigma)
        return noisy, sigma
    d_in, d_out = ctx.malloc(max(flat.nbytes, 8)), ctx.malloc(max(8 * total, 8))
    try:
        ctx.h2d(d_in, flat)
        ctx.memset(d_out, nb.FILL, max(8 * total, 8))
        ctx.synchronize()
        ctx.noise_pick(d_in, dt, offsets, nbatch, snr, level_of, first, seed, d_out, mem, sigma=sigma)
        ctx.synchronize()
        noisy = np.empty(total)
        ctx.d2h(noisy, d_out)
        ctx.synchronize()
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    return noisy, sigma


@pytest.mark.parametrize("mem", (_lib.MEM_HOST, _lib.MEM_DEVICE))
@pytest.mark.parametrize("dt", DTYPES)
def test_every_utterance_is_its_level_of_the_sweep(ctx, sweeps, dt, mem):
    flat, offsets, levels, sweep_sigma = sweeps[dt]
    noisy, sigma = pick(ctx, flat, dt, offsets, SNR, LEVEL_OF, 0, SEED, mem)
    assert set(LEVEL_OF) == set(range(K + 1))
    for b, l in enumerate(LEVEL_OF):
        s = slice(int(offsets[b]), int(offsets[b + 1]))
        assert bits(noisy[s]).tobytes() == bits(levels[l, s]).tobytes(), (b, l)
        assert bits(sigma[b:b + 1]).tobytes() == bits(sweep_sigma[l, b:b + 1]).tobytes(), (b, l)
        if l < K and LENGTHS[b]:
            assert sigma[b] > 0 and not np.array_equal(noisy[s], np.asarray(flat[s], np.float64))
    # without sigma the device call only enqueues: the same samples
    again, none = pick(ctx, flat, dt, offsets, SNR, LEVEL_OF, 0, SEED, mem, want_sigma=False)
    assert none is None and bits(again).tobytes() == bits(noisy).tobytes()


def test_a_sample_depends_on_the_utterance_number_not_on_the_batch(ctx):
    """Utterances 5 .. 7 of an eight-utterance call, and the same three as a call of their own with first_utterance = 5"""
    lengths = (300, 0, 700, 1100, 64, 2049, 513, 1000)
    levels = np.array([0, 1, 2, 0, 1, 2, 0, 1], np.int32)
    flat, offsets = nb.waves(lengths=lengths, seed=90)
    whole, sig = pick(ctx, flat, _lib.WAVE_I16, offsets, SNR, levels, 0, SEED)
    part_off = (offsets[5:] - offsets[5]).astype(np.int64)
    part, psig = pick(ctx, flat[offsets[5]:], _lib.WAVE_I16, part_off, SNR, levels[5:], 5, SEED)
    assert bits(part).tobytes() == bits(whole[offsets[5]:]).tobytes() and bits(psig).tobytes() == bits(sig[5:]).tobytes()
    moved, _ = pick(ctx, flat[offsets[5]:], _lib.WAVE_I16, part_off, SNR, levels[5:], 4, SEED)
    assert not np.array_equal(moved, part)


@pytest.mark.parametrize("dt", DTYPES)
def test_clean_calls_convert_exactly(ctx, dt):
    flat, offsets = nb.waves(dt)
    want = np.asarray(flat, np.float64)
    for snr, level_of in (((), None), (SNR, None), ((), np.zeros(B, np.int32)), (SNR, np.full(B, K, np.int32))):
        noisy, sigma = pick(ctx, flat, dt, offsets, snr, level_of, 0, SEED)
        assert bits(noisy).tobytes() == bits(want).tobytes() and not sigma.any()


def test_equal_values_of_both_dtypes_give_the_same_noise_where_sigma_agrees(ctx):
    """int16 samples and the same values as float64: sigma comes from an exact int64 sum in one case and a float64 sum in the
    other, so it is compared loosely; where it is bit-equal the samples are too, and the deviates are the same everywhere"""
    flat, offsets = nb.waves(_lib.WAVE_I16)
    a, sa = pick(ctx, flat, _lib.WAVE_I16, offsets, SNR, LEVEL_OF, 0, SEED)
    b, sb = pick(ctx, flat.astype(np.float64), _lib.WAVE_F64, offsets, SNR, LEVEL_OF, 0, SEED)
    np.testing.assert_allclose(sa, sb, rtol=1e-12)
    for u in range(B):
        s = slice(int(offsets[u]), int(offsets[u + 1]))
        if sa[u] == sb[u]:
            assert bits(a[s]).tobytes() == bits(b[s]).tobytes(), u
        elif sa[u]:
            np.testing.assert_allclose((a[s] - flat[s]) / sa[u], (b[s] - flat[s]) / sb[u], rtol=0, atol=1e-9)


def test_second_call_same_bytes_other_seed_other_noise(ctx):
    flat, offsets = nb.waves()
    a, sa = pick(ctx, flat, _lib.WAVE_I16, offsets, SNR, LEVEL_OF, 0, SEED)
    b, sb = pick(ctx, flat, _lib.WAVE_I16, offsets, SNR, LEVEL_OF, 0, SEED)
    c, sc = pick(ctx, flat, _lib.WAVE_I16, offsets, SNR, LEVEL_OF, 0, SEED + 1)
    assert bits(a).tobytes() == bits(b).tobytes() and bits(sa).tobytes() == bits(sb).tobytes() == bits(sc).tobytes()
    for u, l in enumerate(LEVEL_OF):
        s = slice(int(offsets[u]), int(offsets[u + 1]))
        assert np.array_equal(a[s], c[s]) == (l == K or LENGTHS[u] == 0), u


def test_empty_calls(ctx):
    flat, offsets = nb.waves()
    noisy, sigma = filled(4, np.float64), filled(4, np.float64)
    assert ctx.lib.f2_noise_pick(ctx.handle, None, _lib.WAVE_I16, None, 0, None, 0, None, 0, 0, None, None, _lib.MEM_HOST) == _lib.F2_OK
    zeros = np.zeros(5, np.int64)
    lev = np.zeros(4, np.int32)
    snr = np.array(SNR)
    assert ctx.lib.f2_noise_pick(ctx.handle, None, _lib.WAVE_I16, ptr(zeros), 4, ptr(snr), K, ptr(lev), 0, 0, ptr(noisy), ptr(sigma),
                                 _lib.MEM_HOST) == _lib.F2_OK
    assert (bits(noisy) == nb.FILL).all() and not sigma.any()


def test_errors_leave_the_outputs_alone(ctx):
    flat, offsets = nb.waves()
    total = int(offsets[-1])
    snr, lev = np.array(SNR), np.array(LEVEL_OF, np.int32)
    noisy, sigma = filled(total, np.float64), filled(B, np.float64)

    def call(wave=flat, dt=_lib.WAVE_I16, off=offsets, nbatch=B, s=snr, k=K, lv=lev, first=0, mem=_lib.MEM_HOST, out=noisy):
        return ctx.lib.f2_noise_pick(ctx.handle, ptr(wave), dt, ptr(off), nbatch, ptr(s), k, ptr(lv), first, SEED, ptr(out), ptr(sigma), mem)

    bad_start, decreasing = offsets.copy(), offsets.copy()
    bad_start[0] = 1
    decreasing[2] = decreasing[1] - 1
    nan_snr = snr.copy()
    nan_snr[1] = np.nan
    inf_snr = snr.copy()
    inf_snr[0] = np.inf
    high, negative = lev.copy(), lev.copy()
    high[4] = K + 1
    negative[2] = -1
    INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    cases = [(dict(dt=7), INV, "wave_dtype"), (dict(mem=5), INV, "mem_space"), (dict(mem=_lib.MEM_HOST_ASYNC), INV, "mem_space"),
             (dict(off=None), INV, "offsets"), (dict(off=bad_start), INV, "offsets[0]"), (dict(off=decreasing), INV, "non-decreasing"),
             (dict(nbatch=-1), INV, "batch"), (dict(s=nan_snr), INV, "snr_db[1]"), (dict(s=inf_snr), INV, "snr_db[0]"),
             (dict(k=-1), INV, "K=-1"), (dict(s=None), INV, "snr_db is NULL"), (dict(lv=high), INV, "utterance 4"),
             (dict(lv=negative), INV, "utterance 2"), (dict(k=2 ** 30), UNS, "levels"), (dict(first=2 ** 32 - B + 1), UNS, "utterance"),
             (dict(wave=None), INV, "null"), (dict(out=None), INV, "null")]
    for kw, code, word in cases:
        rc = call(**kw)
        msg = ctx.lib.f2_last_error(ctx.handle).decode()
        assert rc == code and word in msg, (kw.keys(), rc, msg)
        assert (bits(noisy) == nb.FILL).all() and (bits(sigma) == nb.FILL).all(), kw.keys()
    assert call(first=2 ** 32 - B) == _lib.F2_OK        # the last utterance number that fits
