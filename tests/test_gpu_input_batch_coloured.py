"""f2_input_batch_coloured: the windows of a batch with a room and a coloured-noise level per utterance in one call, against the
three stateless calls it is made of - f2_reverb_pick, then f2_shaped_noise_pick(F2_WAVE_F64) on its output, then
f2_input_batch(F2_WAVE_F64) on that - on raw bytes; against f2_input_batch_wet without filters; and against f2_input_batch on the
pick alone without rooms. The six utterances of tests/noisy_batch.py, windows of 13 x 40."""
import numpy as np
import pytest

import noisy_batch as nb
from f2cnn_amd import _lib
from f2cnn_amd.reverb import SyntheticRIR
from noisy_batch import B, C, K, LEVEL_OF, R, RADIUS, SEED, SNR, STEP, bits, ptr
from test_gpu_shaped_noise import random_filter

pytestmark = pytest.mark.gpu

RIRS = [SyntheticRIR(1.0, t, seed=6, level=l) for l, t in enumerate((7, 1025, 2500))]
KR = len(RIRS)
ROOM_OF = (1, 3, 0, 2, 0, 1)
FIRS = [random_filter(t, 6) for t in (5, 1025, 2048)]
FIRST = 7


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    with c.options(spectral_min_rows=0):        # the 1 s row takes the spectral route in every call of this module
        yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return nb.coefs()


def coloured_windows(ctx, coefs, flat, dt, offsets, lpf, normalize, rirs, room_of, snr, firs, level_of, mem=_lib.MEM_HOST):
    cs, coff = nb.centers()
    out = np.full((int(coff[-1]), R, C), np.nan, np.float32)
    args = (offsets, coefs, B, C, bool(lpf), float(lpf), _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP, normalize, rirs, room_of, snr,
            firs, level_of, FIRST, SEED)
    if mem == _lib.MEM_HOST:
        ctx.input_batch_coloured(flat, dt, *args, out, mem)
        return out
    d_in, d_out = ctx.malloc(flat.nbytes), ctx.malloc(out.nbytes)
    try:
        ctx.h2d(d_in, flat)
        ctx.h2d(d_out, out)
        ctx.synchronize()
        ctx.input_batch_coloured(d_in, dt, *args, d_out, mem)
        ctx.synchronize()
        ctx.d2h(out, d_out)
        ctx.synchronize()
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    return out


def input_batch(ctx, coefs, wave, offsets, lpf, normalize):
    cs, coff = nb.centers()
    want = np.full((int(coff[-1]), R, C), np.nan, np.float32)
    ctx.input_batch(wave, _lib.WAVE_F64, offsets, coefs, B, C, bool(lpf), float(lpf), _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP,
                    normalize, want, _lib.MEM_HOST)
    return want


CASES = [(50, 1, _lib.MEM_HOST, _lib.WAVE_I16), (0, 0, _lib.MEM_HOST, _lib.WAVE_F64), (50, 1, _lib.MEM_DEVICE, _lib.WAVE_I16),
         (0, 0, _lib.MEM_DEVICE, _lib.WAVE_F64)]


@pytest.mark.parametrize("lpf,normalize,mem,dt", CASES)
def test_one_call_equals_reverb_pick_then_shaped_noise_pick_then_input_batch(ctx, coefs, lpf, normalize, mem, dt):
    flat, offsets = nb.waves(dt)
    got = coloured_windows(ctx, coefs, flat, dt, offsets, lpf, normalize, RIRS, ROOM_OF, SNR, FIRS, LEVEL_OF, mem)
    wet, noisy = np.empty(len(flat)), np.empty(len(flat))
    ctx.reverb_pick(flat, dt, offsets, B, RIRS, ROOM_OF, wet, _lib.MEM_HOST)
    sigma = ctx.shaped_noise_pick(wet, _lib.WAVE_F64, offsets, B, SNR, FIRS, LEVEL_OF, FIRST, SEED, noisy, _lib.MEM_HOST, sigma=True)
    want = input_batch(ctx, coefs, noisy, offsets, lpf, normalize)
    assert len(got) > 0 and np.isfinite(got).all()
    assert bits(got).tobytes() == bits(want).tobytes()
    # sigma is the reverberant signal's
    for b, l in enumerate(LEVEL_OF):
        x = wet[offsets[b]:offsets[b + 1]]
        assert sigma[b] == 0 if l == K or not len(x) else np.isclose(sigma[b], np.sqrt(np.mean(x * x)) / 10 ** (SNR[l] / 10), rtol=1e-12)
    # the colours are there: white noise at the same levels gives other windows
    white = coloured_windows(ctx, coefs, flat, dt, offsets, lpf, normalize, RIRS, ROOM_OF, SNR, None, LEVEL_OF, mem)
    assert not np.array_equal(white, got)


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_without_filters_it_is_input_batch_wet(ctx, coefs, dt):
    flat, offsets = nb.waves(dt)
    cs, coff = nb.centers()
    want = np.full((int(coff[-1]), R, C), np.nan, np.float32)
    ctx.input_batch_wet(flat, dt, offsets, coefs, B, C, True, 50.0, _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP, True, RIRS, ROOM_OF, SNR,
                        LEVEL_OF, FIRST, SEED, want, _lib.MEM_HOST)
    got = coloured_windows(ctx, coefs, flat, dt, offsets, 50, 1, RIRS, ROOM_OF, SNR, None, LEVEL_OF)
    assert bits(got).tobytes() == bits(want).tobytes()
    # one-tap filters of 1.0 are white noise too
    got = coloured_windows(ctx, coefs, flat, dt, offsets, 50, 1, RIRS, ROOM_OF, SNR, [np.ones(1)] * K, LEVEL_OF)
    assert bits(got).tobytes() == bits(want).tobytes()


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_without_rooms_it_is_input_batch_on_the_pick_alone(ctx, coefs, dt):
    """the noise stage then reads the waves themselves: the sigma of int16 samples is the int64 one"""
    flat, offsets = nb.waves(dt)
    noisy = np.empty(len(flat))
    ctx.shaped_noise_pick(flat, dt, offsets, B, SNR, FIRS, LEVEL_OF, FIRST, SEED, noisy, _lib.MEM_HOST)
    want = input_batch(ctx, coefs, noisy, offsets, 50, 1)
    for rirs, room_of in (((), None), (RIRS, None), ((), (0,) * B)):
        got = coloured_windows(ctx, coefs, flat, dt, offsets, 50, 1, rirs, room_of, SNR, FIRS, LEVEL_OF)
        assert bits(got).tobytes() == bits(want).tobytes(), (len(rirs), room_of)


def test_errors_of_each_stage_come_before_any_launch(ctx, coefs):
    flat, offsets = nb.waves(_lib.WAVE_I16)
    cs, coff = nb.centers()
    cen = np.concatenate(cs)
    out = nb.filled((int(coff[-1]), R, C), np.float32)
    rir, ro = _lib._pack_rirs(RIRS)
    fir, fo = _lib._pack_rirs(FIRS)
    snr = np.array(SNR)

    def call(rir=rir, ro=ro, kr=KR, room=np.array(ROOM_OF, np.int32), level=np.array(LEVEL_OF, np.int32), fir=fir, fo=fo, centres=cen):
        return ctx.lib.f2_input_batch_coloured(ctx.handle, ptr(flat), _lib.WAVE_I16, ptr(offsets), ptr(coefs), B, C, 0, 0.0, _lib.FFT_F32,
                                               ptr(coff), ptr(centres), RADIUS, STEP, 1, ptr(rir), ptr(ro), kr, ptr(room), ptr(snr), ptr(fir),
                                               ptr(fo), K, ptr(level), FIRST, SEED, ptr(out), _lib.MEM_HOST)
    bad_room, bad_level, nan_rir, nan_fir, far, fo_long = (np.array(ROOM_OF, np.int32), np.array(LEVEL_OF, np.int32), rir.copy(), fir.copy(),
                                                           cen.copy(), fo.copy())
    bad_room[4], bad_level[1], nan_rir[5], nan_fir[2], far[0], fo_long[3] = KR + 1, K + 1, np.nan, np.nan, 0, fo[2] + 2049
    INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    for kw, status, word in ((dict(centres=far), INV, "utterance 0"), (dict(level=bad_level), INV, "utterance 1"),
                             (dict(fo=None), INV, "fir_offsets"), (dict(fir=nan_fir), INV, "level 0"),
                             (dict(fir=np.ones(fo_long[3]), fo=fo_long), UNS, "level 2"),
                             (dict(room=bad_room), INV, "utterance 4"), (dict(rir=None), INV, "rir is NULL"), (dict(rir=nan_rir), INV, "not finite")):
        assert call(**kw) == status, list(kw)
        assert word in ctx.lib.f2_last_error(ctx.handle).decode(), (list(kw), ctx.lib.f2_last_error(ctx.handle).decode())
        assert (bits(out) == nb.FILL).all(), list(kw)
    assert call() == _lib.F2_OK and np.isfinite(out).all()
