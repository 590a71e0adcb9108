"""f2_input_batch_wet: the windows of a batch with a room and a noise level per utterance in one call, against the three stateless
calls it is made of - f2_reverb_pick, then f2_noise_pick(F2_WAVE_F64) on its output, then f2_input_batch(F2_WAVE_F64) on that - on
raw bytes, and against f2_input_batch_noisy where there are no rooms. Windows of 13 x 40 (tests/noisy_batch.py); utterances just
long enough for one, two and three windows, one without centres, and one that reaches into a second tile of the kernel."""
import numpy as np
import pytest

import noisy_batch as nb
from f2cnn_amd import _lib
from f2cnn_amd.reverb import SyntheticRIR
from noisy_batch import C, R, RADIUS, REACH, SEED, SNR, STEP, bits, ptr

pytestmark = pytest.mark.gpu

W = 2 * REACH + 1                                   # samples of one window
LENGTHS = (W, W + 1, 30, W + 2, _lib.REVERB_BLOCK + 6)
B = len(LENGTHS)
RIRS = [SyntheticRIR(1.0, t, seed=6, level=l) for l, t in enumerate((1, 1025, 2500))]
KR, K = len(RIRS), len(SNR)
ROOM_OF = (2, 3, 0, 1, 1)
LEVEL_OF = (0, 1, 2, 3, 2)
FIRST = 7


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return nb.coefs()


def centres():
    """every legal centre of the short utterances (one, two, none, three), the first and the last of the long one"""
    cs = [np.arange(REACH, n - REACH, dtype=np.int64) for n in LENGTHS[:4]] + [np.array([REACH, LENGTHS[4] - 1 - REACH], np.int64)]
    assert [len(c) for c in cs] == [1, 2, 0, 3, 2]
    return cs, np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)


def wet_windows(ctx, coefs, flat, dt, offsets, lpf, normalize, rirs, room_of, snr, level_of, mem=_lib.MEM_HOST):
    cs, coff = centres()
    out = np.full((int(coff[-1]), R, C), np.nan, np.float32)
    args = (offsets, coefs, B, C, bool(lpf), float(lpf), _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP, normalize, rirs, room_of, snr,
            level_of, FIRST, SEED)
    if mem == _lib.MEM_HOST:
        ctx.input_batch_wet(flat, dt, *args, out, mem)
        return out
    d_in, d_out = ctx.malloc(flat.nbytes), ctx.malloc(out.nbytes)
    try:
        ctx.h2d(d_in, flat)
        ctx.h2d(d_out, out)
        ctx.synchronize()
        ctx.input_batch_wet(d_in, dt, *args, d_out, mem)
        ctx.synchronize()
        ctx.d2h(out, d_out)
        ctx.synchronize()
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    return out


CASES = [(lpf, norm, _lib.MEM_HOST, dt) for lpf in (0, 50) for norm in (0, 1) for dt in (_lib.WAVE_I16, _lib.WAVE_F64)]
CASES += [(50, 1, _lib.MEM_DEVICE, _lib.WAVE_I16), (0, 0, _lib.MEM_DEVICE, _lib.WAVE_F64)]


@pytest.mark.parametrize("lpf,normalize,mem,dt", CASES)
def test_one_call_equals_reverb_pick_then_noise_pick_then_input_batch(ctx, coefs, lpf, normalize, mem, dt):
    flat, offsets = nb.waves(dt, LENGTHS, seed=80)
    cs, coff = centres()
    got = wet_windows(ctx, coefs, flat, dt, offsets, lpf, normalize, RIRS, ROOM_OF, SNR, LEVEL_OF, mem)
    wet, noisy = np.empty(len(flat)), np.empty(len(flat))
    ctx.reverb_pick(flat, dt, offsets, B, RIRS, ROOM_OF, wet, _lib.MEM_HOST)
    sigma = ctx.noise_pick(wet, _lib.WAVE_F64, offsets, B, SNR, LEVEL_OF, FIRST, SEED, noisy, _lib.MEM_HOST, sigma=True)
    want = np.full(got.shape, np.nan, np.float32)
    ctx.input_batch(noisy, _lib.WAVE_F64, offsets, coefs, B, C, bool(lpf), float(lpf), _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP,
                    normalize, want, _lib.MEM_HOST)
    assert len(got) == coff[-1] == 8 and np.isfinite(got).all()
    assert bits(got).tobytes() == bits(want).tobytes()
    # sigma is the reverberant signal's: the float64 rule on `wet`, not the clean utterance's
    for b, l in enumerate(LEVEL_OF):
        x = wet[offsets[b]:offsets[b + 1]]
        assert sigma[b] == 0 if l == K else np.isclose(sigma[b], np.sqrt(np.mean(x * x)) / 10 ** (SNR[l] / 10), rtol=1e-12)
    # rooms without noise, and noise among rooms that are all the dry one
    only_rooms = wet_windows(ctx, coefs, flat, dt, offsets, lpf, normalize, RIRS, ROOM_OF, (), None, mem)
    ctx.input_batch(wet, _lib.WAVE_F64, offsets, coefs, B, C, bool(lpf), float(lpf), _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP,
                    normalize, want, _lib.MEM_HOST)
    assert bits(only_rooms).tobytes() == bits(want).tobytes() and not np.array_equal(only_rooms, got)


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_without_rooms_it_is_input_batch_noisy(ctx, coefs, dt):
    flat, offsets = nb.waves(dt, LENGTHS, seed=80)
    cs, coff = centres()
    want = np.full((int(coff[-1]), R, C), np.nan, np.float32)
    ctx.input_batch_noisy(flat, dt, offsets, coefs, B, C, True, 50.0, _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP, True, SNR,
                          LEVEL_OF, FIRST, SEED, want, _lib.MEM_HOST)
    for rirs, room_of in (((), None), (RIRS, None), ((), (0,) * B)):
        got = wet_windows(ctx, coefs, flat, dt, offsets, 50, 1, rirs, room_of, SNR, LEVEL_OF)
        assert bits(got).tobytes() == bits(want).tobytes(), (len(rirs), room_of)


def test_errors_come_before_any_launch(ctx, coefs):
    flat, offsets = nb.waves(_lib.WAVE_I16, LENGTHS, seed=80)
    cs, coff = centres()
    cen = np.concatenate(cs)
    out = nb.filled((int(coff[-1]), R, C), np.float32)
    rir = np.concatenate(RIRS)
    ro = np.concatenate([[0], np.cumsum([len(h) for h in RIRS])]).astype(np.int64)
    snr = np.array(SNR)

    def call(rir=rir, ro=ro, kr=KR, room=np.array(ROOM_OF, np.int32), level=np.array(LEVEL_OF, np.int32)):
        return ctx.lib.f2_input_batch_wet(ctx.handle, ptr(flat), _lib.WAVE_I16, ptr(offsets), ptr(coefs), B, C, 0, 0.0, _lib.FFT_F32, ptr(coff),
                                          ptr(cen), RADIUS, STEP, 1, ptr(rir), ptr(ro), kr, ptr(room), ptr(snr), K, ptr(level), FIRST, SEED,
                                          ptr(out), _lib.MEM_HOST)
    bad_room, bad_level, nan_tap = np.array(ROOM_OF, np.int32), np.array(LEVEL_OF, np.int32), rir.copy()
    bad_room[4], bad_level[1], nan_tap[5] = KR + 1, K + 1, np.nan
    for kw, word in ((dict(room=bad_room), "utterance 4"), (dict(level=bad_level), "utterance 1"), (dict(rir=None), "rir is NULL"),
                     (dict(kr=-1), "K=-1"), (dict(rir=nan_tap), "not finite")):
        assert call(**kw) == _lib.F2_ERR_INVALID, kw.keys()
        assert word in ctx.lib.f2_last_error(ctx.handle).decode(), kw.keys()
        assert (bits(out) == nb.FILL).all(), kw.keys()
    assert call() == _lib.F2_OK and np.isfinite(out).all()
