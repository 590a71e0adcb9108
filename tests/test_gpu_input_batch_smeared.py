"""f2_input_batch_smeared: the windows of a batch with a room, a coloured-noise level and a spectral resolution per utterance in one
call, against the four stateless calls it is made of - f2_reverb_pick, f2_shaped_noise_pick(F2_WAVE_F64) on its output,
f2_filterbank_envelope_fused(F2_WAVE_F64, gfb NULL) on that, f2_gather_windows_mixed on those envelopes - on raw bytes; against
f2_input_batch_coloured without matrices; the whole ladder of entries on one small batch; and the errors of each stage, which come
before any launch. Three utterances of 0.2 to 0.4 s, 32 channels, windows of 11 x 32."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib, smear
from f2cnn_amd.reverb import SyntheticRIR
from noisy_batch import FILL, bits, filled, ptr
from test_gpu_shaped_noise import random_filter

pytestmark = pytest.mark.gpu

C, RADIUS, STEP = 32, 5, 160
R, REACH = 2 * RADIUS + 1, RADIUS * STEP
LENGTHS = (3200, 6400, 4801)
B = len(LENGTHS)
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
RIRS = [SyntheticRIR(1.0, t, seed=6, level=l) for l, t in enumerate((7, 1025))]
ROOM_OF = (1, 2, 0)
SNR = (20.0, 3.0)
FIRS = [random_filter(t, 6) for t in (5, 1025)]
LEVEL_OF = (0, 2, 1)
K, KR, KM = len(SNR), len(RIRS), 3
MIX_OF = (1, 3, 0)
FIRST, SEED = 7, 0x1234_5678_9ABC


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))


def waves(dt):
    flat = np.concatenate([orc.synth_utterance(80 + i, n) for i, n in enumerate(LENGTHS)]).astype(np.int16)
    return flat if dt == _lib.WAVE_I16 else flat.astype(np.float64) * 0.37


def centres():
    rng = np.random.default_rng(5)
    cs = []
    for n in LENGTHS:
        c = rng.integers(REACH, n - REACH, size=4).astype(np.int64)
        c[0], c[-1] = REACH, n - 1 - REACH
        cs.append(c)
    return np.concatenate(cs), np.arange(B + 1, dtype=np.int64) * 4


def matrices():
    freqs = orc.centre_freqs(16000, C, 100)
    return np.stack([smear.SmearMatrix(freqs, 2.0), smear.BandMatrix(C, 4), smear.SmearMatrix(freqs, 0.5)])


def smeared_windows(ctx, coefs, flat, dt, lpf, normalize, rirs, room_of, snr, firs, level_of, mixes, mix_of, mem=_lib.MEM_HOST, call=None):
    cen, coff = centres()
    out = np.full((int(coff[-1]), R, C), np.nan, np.float32)
    args = (OFFSETS, coefs, B, C, bool(lpf), float(lpf), _lib.FFT_F32, coff, cen, RADIUS, STEP, normalize, rirs, room_of, snr, firs, level_of,
            FIRST, SEED)
    tail = () if call else (mixes, mix_of)
    call = call or ctx.input_batch_smeared
    if mem == _lib.MEM_HOST:
        call(flat, dt, *args, *tail, out, mem)
        return out
    d_in, d_out = ctx.malloc(flat.nbytes), ctx.malloc(out.nbytes)
    try:
        ctx.h2d(d_in, flat)
        ctx.h2d(d_out, out)
        ctx.synchronize()
        call(d_in, dt, *args, *tail, d_out, mem)
        ctx.synchronize()
        ctx.d2h(out, d_out)
        ctx.synchronize()
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    return out


CASES = [(50, 1, _lib.MEM_HOST, _lib.WAVE_I16), (0, 0, _lib.MEM_HOST, _lib.WAVE_F64), (50, 1, _lib.MEM_DEVICE, _lib.WAVE_F64),
         (0, 0, _lib.MEM_DEVICE, _lib.WAVE_I16)]


@pytest.mark.parametrize("lpf,normalize,mem,dt", CASES)
def test_one_call_equals_its_four_stages(ctx, coefs, lpf, normalize, mem, dt):
    flat, mix = waves(dt), matrices()
    got = smeared_windows(ctx, coefs, flat, dt, lpf, normalize, RIRS, ROOM_OF, SNR, FIRS, LEVEL_OF, mix, MIX_OF, mem)
    wet, noisy, env = np.empty(len(flat)), np.empty(len(flat)), np.empty(C * len(flat))
    ctx.reverb_pick(flat, dt, OFFSETS, B, RIRS, ROOM_OF, wet, _lib.MEM_HOST)
    ctx.shaped_noise_pick(wet, _lib.WAVE_F64, OFFSETS, B, SNR, FIRS, LEVEL_OF, FIRST, SEED, noisy, _lib.MEM_HOST)
    ctx.filterbank_envelope_fused(noisy, _lib.WAVE_F64, OFFSETS, coefs, B, C, bool(lpf), float(lpf), _lib.FFT_F32, env, None, _lib.MEM_HOST)
    cen, coff = centres()
    want = np.full_like(got, np.nan)
    ctx.gather_windows_mixed(env, OFFSETS, B, C, coff, cen, RADIUS, STEP, normalize, mix, MIX_OF, want, _lib.MEM_HOST)
    assert len(got) > 0 and np.isfinite(got).all()
    assert bits(got).tobytes() == bits(want).tobytes()
    # the mixing is there: the same call at full resolution gives other windows
    sharp = smeared_windows(ctx, coefs, flat, dt, lpf, normalize, RIRS, ROOM_OF, SNR, FIRS, LEVEL_OF, None, None, mem)
    assert not np.array_equal(sharp[:8], got[:8]) and bits(sharp[4:8]).tobytes() == bits(got[4:8]).tobytes()   # (utterance 1 is sharp)


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_without_matrices_it_is_input_batch_coloured(ctx, coefs, dt):
    flat, mix = waves(dt), matrices()
    want = smeared_windows(ctx, coefs, flat, dt, 50, 1, RIRS, ROOM_OF, SNR, FIRS, LEVEL_OF, None, None, call=ctx.input_batch_coloured)
    for mixes, mix_of in ((None, None), (mix, None), (None, (0,) * B), (mix, (KM,) * B)):
        got = smeared_windows(ctx, coefs, flat, dt, 50, 1, RIRS, ROOM_OF, SNR, FIRS, LEVEL_OF, mixes, mix_of)
        assert bits(got).tobytes() == bits(want).tobytes(), mix_of
    # ... and the stages compose: no rooms, no noise, matrices alone
    got = smeared_windows(ctx, coefs, flat, dt, 50, 1, (), None, (), None, None, mix, MIX_OF)
    env = np.empty(C * len(flat))
    ctx.filterbank_envelope_fused(flat, dt, OFFSETS, coefs, B, C, True, 50.0, _lib.FFT_F32, env, None, _lib.MEM_HOST)
    cen, coff = centres()
    alone = np.full_like(got, np.nan)
    ctx.gather_windows_mixed(env, OFFSETS, B, C, coff, cen, RADIUS, STEP, True, mix, MIX_OF, alone, _lib.MEM_HOST)
    assert bits(got).tobytes() == bits(alone).tobytes()


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_the_whole_ladder_gives_the_same_bytes(ctx, dt):
    """A configuration a lower entry can express gives the same bytes through every higher one: f2_input_batch_noisy through _wet,
    _coloured and _smeared, _wet through _coloured and _smeared, _coloured through _smeared (the other tests compare neighbours
    only). 8 channels, utterances of 1761, 2500 and 1000 samples - the last without room for a window."""
    lens, Cs = (1761, 2500, 1000), 8
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.concatenate([orc.synth_utterance(90 + i, n) for i, n in enumerate(lens)]).astype(np.int16)
    flat = flat if dt == _lib.WAVE_I16 else flat.astype(np.float64) * 0.37
    small = orc.make_erb_filters(16000, orc.centre_freqs(16000, Cs, 100))
    cs = [np.array([REACH, n // 2, n - 1 - REACH], np.int64) if n > 2 * REACH else np.zeros(0, np.int64) for n in lens]
    cen, coff = np.concatenate(cs), np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    entries = ("noisy", "wet", "coloured", "smeared")

    def through(entry, rooms, firs):
        noise = (LEVEL_OF, FIRST, SEED)
        stages = {"noisy": (SNR, *noise), "wet": (*rooms, SNR, *noise), "coloured": (*rooms, SNR, firs, *noise),
                  "smeared": (*rooms, SNR, firs, *noise, None, None)}[entry]
        out = np.full((int(coff[-1]), R, Cs), np.nan, np.float32)
        getattr(ctx, "input_batch_" + entry)(flat, dt, offs, small, len(lens), Cs, True, 50.0, _lib.FFT_F32, coff, cen, RADIUS, STEP, True,
                                             *stages, out, _lib.MEM_HOST)
        assert len(out) == 6 and np.isfinite(out).all()
        return out
    seen = []
    for lowest, rooms, firs in (("noisy", ((), None), None), ("wet", (RIRS, ROOM_OF), None), ("coloured", (RIRS, ROOM_OF), FIRS)):
        want = through(lowest, rooms, firs)
        for higher in entries[entries.index(lowest) + 1:]:
            assert bits(through(higher, rooms, firs)).tobytes() == bits(want).tobytes(), (lowest, higher)
        seen.append(want)
    # ... and the three configurations are three: a room and a colour each change the windows of utterance 0
    assert not np.array_equal(seen[0][:3], seen[1][:3]) and not np.array_equal(seen[1][:3], seen[2][:3])


def test_errors_of_each_stage_come_before_any_launch(ctx, coefs):
    flat, mix = waves(_lib.WAVE_I16), matrices()
    cen, coff = centres()
    out = filled((int(coff[-1]), R, C), np.float32)
    rir, ro = _lib._pack_rirs(RIRS)
    fir, fo = _lib._pack_rirs(FIRS)
    snr = np.array(SNR)

    def call(rir=rir, room=np.array(ROOM_OF, np.int32), level=np.array(LEVEL_OF, np.int32), fir=fir, centres=cen, mix=mix, km=KM,
             mix_of=np.array(MIX_OF, np.int32)):
        return ctx.lib.f2_input_batch_smeared(ctx.handle, ptr(flat), _lib.WAVE_I16, ptr(OFFSETS), ptr(coefs), B, C, 0, 0.0, _lib.FFT_F32,
                                              ptr(coff), ptr(centres), RADIUS, STEP, 1, ptr(rir), ptr(ro), KR, ptr(room), ptr(snr), ptr(fir),
                                              ptr(fo), K, ptr(level), FIRST, SEED, ptr(mix), km, ptr(mix_of), ptr(out), _lib.MEM_HOST)
    bad_room, bad_level, nan_fir, far, nan_mix, bad_mix_of = (np.array(ROOM_OF, np.int32), np.array(LEVEL_OF, np.int32), fir.copy(), cen.copy(),
                                                              mix.copy(), np.array(MIX_OF, np.int32))
    bad_room[2], bad_level[1], nan_fir[2], far[0], nan_mix[1, 4, 5], bad_mix_of[2] = KR + 1, K + 1, np.nan, 0, np.nan, KM + 1
    INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    for kw, status, word in ((dict(centres=far), INV, "utterance 0"), (dict(level=bad_level), INV, "utterance 1"),
                             (dict(fir=nan_fir), INV, "level 0"), (dict(room=bad_room), INV, "utterance 2"), (dict(rir=None), INV, "rir is NULL"),
                             (dict(mix=None), INV, "mixing"), (dict(mix=nan_mix), INV, "[1][4][5]"), (dict(mix_of=bad_mix_of), INV, "utterance 2"),
                             (dict(km=-1), INV, "K=-1"), (dict(mix=np.resize(mix, (65, C, C)), km=65), UNS, "65 mixing matrices")):
        assert call(**kw) == status, list(kw)
        assert word in ctx.lib.f2_last_error(ctx.handle).decode(), (list(kw), ctx.lib.f2_last_error(ctx.handle).decode())
        assert (bits(out) == FILL).all(), list(kw)
    assert call() == _lib.F2_OK and np.isfinite(out).all()
