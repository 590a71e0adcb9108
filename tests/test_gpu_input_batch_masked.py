"""f2_input_batch_masked and f2_trainer_render_masked: a recorded masker per utterance between the room and the noise. The one call
against the stateless calls it is made of - f2_reverb_pick, f2_masker_pick(F2_WAVE_F64) on its output, f2_input_batch_smeared
(F2_WAVE_F64, no rooms) on that - on raw bytes; without maskers against f2_input_batch_smeared; a render in groups of two over five
utterances against f2_input_batch_masked per group; and the errors of the stage, which come before any launch. The batch, rooms,
colours and matrices of tests/test_gpu_input_batch_smeared.py."""
import numpy as np
import pytest

import masker_cases as mc
import noisy_batch as nb
import train_referee as tr
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.trainer import Trainer
from noisy_batch import FILL, bits, filled, ptr
from test_gpu_input_batch_smeared import (B, C, FIRS, FIRST, K, KM, KR, LEVEL_OF, MIX_OF, OFFSETS, R, RADIUS, RIRS, ROOM_OF, SEED, SNR, STEP,
                                          centres, matrices, waves)

pytestmark = pytest.mark.gpu

MASKERS, MASKER_OF, MASKER_SNRS = mc.SETS["wraps"]
KK = len(MASKER_SNRS)
MASKER_LEVEL_OF = (4, 5, 1)                        # the long recording, none, the one of 7 samples


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    import f2cnn_oracle as orc
    return orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))


def masked_windows(ctx, coefs, flat, dt, lpf, normalize, rirs, room_of, snr, firs, level_of, mixes, mix_of, maskers, masker_of, masker_snrs,
                   masker_level_of, mem=_lib.MEM_HOST, call=None):
    cen, coff = centres()
    out = np.full((int(coff[-1]), R, C), np.nan, np.float32)
    args = (OFFSETS, coefs, B, C, bool(lpf), float(lpf), _lib.FFT_F32, coff, cen, RADIUS, STEP, normalize, rirs, room_of, snr, firs, level_of,
            FIRST, SEED, mixes, mix_of)
    tail = () if call else (maskers, masker_of, masker_snrs, masker_level_of)
    call = call or ctx.input_batch_masked
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


CASES = [(50, 1, _lib.MEM_HOST, _lib.WAVE_I16, True), (0, 0, _lib.MEM_HOST, _lib.WAVE_F64, True), (50, 1, _lib.MEM_DEVICE, _lib.WAVE_F64, False),
         (0, 0, _lib.MEM_DEVICE, _lib.WAVE_I16, False)]


@pytest.mark.parametrize("lpf,normalize,mem,dt,rooms", CASES)
def test_one_call_equals_its_stages(ctx, coefs, lpf, normalize, mem, dt, rooms):
    flat, mix = waves(dt), matrices()
    rirs, room_of = (RIRS, ROOM_OF) if rooms else ((), None)
    got = masked_windows(ctx, coefs, flat, dt, lpf, normalize, rirs, room_of, SNR, FIRS, LEVEL_OF, mix, MIX_OF, MASKERS, MASKER_OF, MASKER_SNRS,
                         MASKER_LEVEL_OF, mem)
    wet, masked = np.empty(len(flat)), np.empty(len(flat))
    ctx.reverb_pick(flat, dt, OFFSETS, B, rirs, room_of, wet, _lib.MEM_HOST)
    _, gain, _ = ctx.masker_pick(wet, _lib.WAVE_F64, OFFSETS, B, MASKER_SNRS, MASKERS, MASKER_OF, MASKER_LEVEL_OF, FIRST, SEED, masked,
                                 _lib.MEM_HOST, small=True)
    want = masked_windows(ctx, coefs, masked, _lib.WAVE_F64, lpf, normalize, (), None, SNR, FIRS, LEVEL_OF, mix, MIX_OF, None, None, (), None,
                          call=ctx.input_batch_smeared)
    assert len(got) > 0 and np.isfinite(got).all()
    assert bits(got).tobytes() == bits(want).tobytes()
    # the maskers are there: utterances 0 and 2 have one, utterance 1 has none
    assert gain[0] > 0 and gain[1] == 0 and gain[2] > 0
    bare = masked_windows(ctx, coefs, flat, dt, lpf, normalize, rirs, room_of, SNR, FIRS, LEVEL_OF, mix, MIX_OF, None, None, (), None, mem)
    assert not np.array_equal(bare[:4], got[:4]) and not np.array_equal(bare[8:], got[8:]) and bits(bare[4:8]).tobytes() == bits(got[4:8]).tobytes()


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_without_maskers_it_is_input_batch_smeared(ctx, coefs, dt):
    flat, mix = waves(dt), matrices()
    stages = (RIRS, ROOM_OF, SNR, FIRS, LEVEL_OF, mix, MIX_OF)
    want = masked_windows(ctx, coefs, flat, dt, 50, 1, *stages, None, None, (), None, call=ctx.input_batch_smeared)
    for maskers, masker_of, snrs, level_of in ((None, None, (), None), (MASKERS, MASKER_OF, MASKER_SNRS, None),
                                               (MASKERS, MASKER_OF, MASKER_SNRS, (KK,) * B), (None, None, (), (0,) * B)):
        got = masked_windows(ctx, coefs, flat, dt, 50, 1, *stages, maskers, masker_of, snrs, level_of)
        assert bits(got).tobytes() == bits(want).tobytes(), level_of
    # ... and the stage composes with nothing around it: maskers alone are f2_input_batch on f2_masker_pick's output
    got = masked_windows(ctx, coefs, flat, dt, 50, 1, (), None, (), None, None, None, None, MASKERS, MASKER_OF, MASKER_SNRS, MASKER_LEVEL_OF)
    masked = np.empty(len(flat))
    ctx.masker_pick(flat, dt, OFFSETS, B, MASKER_SNRS, MASKERS, MASKER_OF, MASKER_LEVEL_OF, FIRST, SEED, masked, _lib.MEM_HOST)
    cen, coff = centres()
    alone = np.full_like(got, np.nan)
    ctx.input_batch(masked, _lib.WAVE_F64, OFFSETS, coefs, B, C, True, 50.0, _lib.FFT_F32, coff, cen, RADIUS, STEP, True, alone, _lib.MEM_HOST)
    assert bits(got).tobytes() == bits(alone).tobytes() and not np.array_equal(got, want)


def test_errors_of_the_stage_come_before_any_launch(ctx, coefs):
    flat, mix = waves(_lib.WAVE_I16), matrices()
    cen, coff = centres()
    out = filled((int(coff[-1]), R, C), np.float32)
    rir, ro = _lib._pack_rirs(RIRS)
    fir, fo = _lib._pack_rirs(FIRS)
    masker, moff = _lib._pack_rirs(MASKERS)
    snr, msnr = np.array(SNR), np.array(MASKER_SNRS)

    def call(masker=masker, moff=moff, r=len(MASKERS), mof=np.array(MASKER_OF, np.int32), kk=KK, mlev=np.array(MASKER_LEVEL_OF, np.int32),
             msnr=msnr, mix_of=np.array(MIX_OF, np.int32)):
        return ctx.lib.f2_input_batch_masked(ctx.handle, ptr(flat), _lib.WAVE_I16, ptr(OFFSETS), ptr(coefs), B, C, 0, 0.0, _lib.FFT_F32, ptr(coff),
                                             ptr(cen), RADIUS, STEP, 1, ptr(rir), ptr(ro), KR, ptr(np.array(ROOM_OF, np.int32)), ptr(snr),
                                             ptr(fir), ptr(fo), K, ptr(np.array(LEVEL_OF, np.int32)), FIRST, SEED, ptr(mix), KM, ptr(mix_of),
                                             ptr(msnr), ptr(masker), ptr(moff), r, ptr(mof), kk, ptr(mlev), ptr(out), _lib.MEM_HOST)
    bad_lev, nan, bad_of, nan_snr, bad_mix_of = (np.array(MASKER_LEVEL_OF, np.int32), masker.copy(), np.array(MASKER_OF, np.int32), msnr.copy(),
                                                 np.array(MIX_OF, np.int32))
    bad_lev[2], nan[9], bad_of[3], nan_snr[1], bad_mix_of[0] = KK + 1, np.inf, 4, np.nan, KM + 1
    INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    for kw, status, word in ((dict(mlev=bad_lev), INV, "utterance 2"), (dict(masker=nan), INV, "recording 2: sample 1"), (dict(mof=bad_of), INV, "level 3"),
                             (dict(msnr=nan_snr), INV, "snr_db[1]"), (dict(masker=None), INV, "masker"), (dict(r=65), UNS, "65 recordings"),
                             (dict(kk=-1), INV, "K=-1"), (dict(mix_of=bad_mix_of), INV, "utterance 0")):
        assert call(**kw) == status, list(kw)
        assert word in ctx.lib.f2_last_error(ctx.handle).decode(), (list(kw), ctx.lib.f2_last_error(ctx.handle).decode())
        assert (bits(out) == FILL).all(), list(kw)
    assert call() == _lib.F2_OK and np.isfinite(out).all()


# ---- the render --------------------------------------------------------------------------------------------------------------
NB, GROUP = 5, 2                                   # the first five utterances of tests/noisy_batch.py: groups of 2, 2 and 1
T_ROOM_OF, T_MIX_OF, T_MASKER_LEVEL_OF = (1, 2, 0, 2, 0), (2, 0, 1, 3, 1), (3, 5, 0, 4, 2)


def test_render_in_groups_is_input_batch_masked_per_group(ctx):
    from test_gpu_train_smear import matrices as train_matrices
    flat, offsets = nb.waves()
    cs, _ = nb.centers()
    cs = cs[:NB]
    rng = np.random.default_rng(3)
    signs = [rng.integers(0, 2, len(c)).astype(np.uint8) for c in cs]
    Ct, Rt = nb.C, nb.R
    coefs, mix = nb.coefs(), train_matrices()
    room, lev, mof, mlev = (np.array(a, np.int32) for a in (T_ROOM_OF, nb.LEVEL_OF[:NB], T_MIX_OF, T_MASKER_LEVEL_OF))
    with ctx.options(spectral_min_rows=0):
        t = Trainer(F2CNNModel.glorot(7, Rt, Ct, zero_bias=False), lr=1e-3, rho=0.9, eps=1e-7, decay=0.5, drop=tr.DROP, seed=5, ctx=ctx)
        t.set_waves([flat[offsets[b]:offsets[b + 1]] for b in range(NB)], cs, signs, coefs, nb.RADIUS, nb.STEP, lpf=True, cutoff=50.0, group=GROUP)
        masking = dict(maskers=MASKERS, masker_of=MASKER_OF, masker_snrs=MASKER_SNRS, masker_level_of=mlev)
        t.render_wet(RIRS, room, nb.SNR, lev, nb.SEED, firs=FIRS[:1] * 3, mixes=mix, mix_of=mof, **masking)
        x, y = t.windows()
        assert np.array_equal(y, np.concatenate(signs)) and np.isfinite(x).all()
        row = 0
        for g in range(0, NB, GROUP):                       # group g starts at first_utterance = g; the last one is partial
            e = min(g + GROUP, NB)
            coff = np.concatenate([[0], np.cumsum([len(c) for c in cs[g:e]])]).astype(np.int64)
            want = np.full((int(coff[-1]), Rt, Ct), np.nan, np.float32)
            if len(want):
                ctx.input_batch_masked(flat[int(offsets[g]):int(offsets[e])], _lib.WAVE_I16, offsets[g:e + 1] - offsets[g], coefs, e - g, Ct, True,
                                       50.0, _lib.FFT_F32, coff, np.concatenate(cs[g:e]), nb.RADIUS, nb.STEP, True, RIRS, room[g:e], nb.SNR,
                                       FIRS[:1] * 3, lev[g:e], g, nb.SEED, mix, mof[g:e], MASKERS, MASKER_OF, MASKER_SNRS, mlev[g:e], want,
                                       _lib.MEM_HOST)
            assert bits(x[row:row + len(want)]).tobytes() == bits(want).tobytes(), g
            row += len(want)
        assert row == len(x)
        # without maskers it is the render it was; a second masked render gives the same bytes; a bad level changes nothing
        t.render_wet(RIRS, room, nb.SNR, lev, nb.SEED, firs=FIRS[:1] * 3, mixes=mix, mix_of=mof)
        old = t.windows()[0]
        ctx.trainer_render_masked(t.handle, RIRS, room, nb.SNR, FIRS[:1] * 3, lev, nb.SEED, mix, mof, Ct, MASKERS, MASKER_OF, MASKER_SNRS, None)
        assert bits(t.windows()[0]).tobytes() == bits(old).tobytes() and not np.array_equal(old, x)
        t.render_wet(RIRS, room, nb.SNR, lev, nb.SEED, firs=FIRS[:1] * 3, mixes=mix, mix_of=mof, **masking)
        assert bits(t.windows()[0]).tobytes() == bits(x).tobytes()
        bad = mlev.copy()
        bad[3] = KK + 1
        with pytest.raises(_lib.F2Error, match="utterance 3") as ei:
            t.render(maskers=MASKERS, masker_of=MASKER_OF, masker_snrs=MASKER_SNRS, masker_level_of=bad)
        assert ei.value.code == _lib.F2_ERR_INVALID and bits(t.windows()[0]).tobytes() == bits(x).tobytes()
        t.close()
