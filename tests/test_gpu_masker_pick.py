"""f2_masker_pick: one masker level per utterance in the layout of the waves, against the level blocks of f2_masker_levels on raw
bits, with first_utterance shifting the draw, the clean cases that need no recording, and the errors, which come before anything is
written. Through the C ABI via ctypes."""
import numpy as np
import pytest

import masker_cases as mc
from f2cnn_amd import _lib
from masker_cases import B, K, LENGTHS, SEED, bits, filled, ptr

pytestmark = pytest.mark.gpu

LEVEL_OF = (2, 5, 0, 4, 1, 3, 4)          # every level and the clean one; the two levels of one recording
INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def pick(ctx, wave, dt, offsets, name, level_of, first=0, seed=SEED):
    recordings, masker_of, snr = mc.SETS[name]
    out = filled(int(offsets[-1]), np.float64)
    small = ctx.masker_pick(wave, dt, offsets, len(offsets) - 1, snr, recordings, masker_of, level_of, first, seed, out, _lib.MEM_HOST, small=True)
    return (out,) + small


@pytest.mark.parametrize("name", list(mc.SETS))
@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_the_pick_is_that_level_of_the_sweep(ctx, name, dt):
    wave, offsets = mc.ragged_waves()
    wave = wave if dt == _lib.WAVE_I16 else wave.astype(np.float64)
    recordings, masker_of, snr = mc.SETS[name]
    total = int(offsets[-1])
    levels = filled((K + 1) * total, np.float64)
    small = ctx.masker_levels(wave, dt, offsets, B, snr, recordings, masker_of, SEED, levels, _lib.MEM_HOST)
    levels = levels.reshape(K + 1, total)
    for shift in range(2):
        level_of = [(l + shift) % (K + 1) for l in LEVEL_OF]
        out, sigma, gain, start = pick(ctx, wave, dt, offsets, name, level_of)
        for b, l in enumerate(level_of):
            assert bits(out[offsets[b]:offsets[b + 1]]).tobytes() == bits(levels[l, offsets[b]:offsets[b + 1]]).tobytes(), (b, l)
            for got, want in zip((sigma, gain, start), small):
                assert bits(got[b:b + 1]).tobytes() == bits(want.reshape(K + 1, B)[l, b:b + 1]).tobytes(), (b, l)


def test_first_utterance_shifts_the_draw(ctx):
    """utterances 3 .. 6 of the batch, picked alone as utterances first_utterance + 0 .. 3, are theirs in the whole batch"""
    wave, offsets = mc.ragged_waves()
    whole = pick(ctx, wave, _lib.WAVE_I16, offsets, "wraps", LEVEL_OF)
    first = 3
    part, off = wave[offsets[first]:], offsets[first:] - offsets[first]
    shifted = pick(ctx, part, _lib.WAVE_I16, off, "wraps", LEVEL_OF[first:], first=first)
    assert bits(shifted[0]).tobytes() == bits(whole[0][offsets[first]:]).tobytes()
    for got, want in zip(shifted[1:], whole[1:]):
        assert bits(got).tobytes() == bits(want[first:]).tobytes()
    # ... and the same utterances numbered from 0 draw other segments
    unshifted = pick(ctx, part, _lib.WAVE_I16, off, "wraps", LEVEL_OF[first:], first=0)
    recordings, masker_of, _ = mc.SETS["wraps"]
    assert not np.array_equal(unshifted[3], shifted[3]) and not np.array_equal(unshifted[0], shifted[0])
    for b, l in enumerate(LEVEL_OF[first:]):
        r = masker_of[l]
        assert int(shifted[3][b]) == mc.start_of(SEED, r, first + b, len(recordings[r]))
        assert int(unshifted[3][b]) == mc.start_of(SEED, r, b, len(recordings[r]))


def test_without_levels_it_converts_and_needs_no_recording(ctx):
    wave, offsets = mc.ragged_waves()
    want = bits(wave.astype(np.float64)).tobytes()
    recordings, masker_of, snr = mc.SETS["wraps"]
    masker, moff = _lib._pack_rirs(recordings)
    snr, mof, clean = np.array(snr, np.float64), np.array(masker_of, np.int32), np.full(B, K, np.int32)
    # no level_of; K = 0; every utterance at the clean level - with the recordings and without
    for k, level, with_maskers in ((K, None, True), (K, None, False), (0, clean * 0, False), (0, None, False), (K, clean, True), (K, clean, False)):
        out, sigma, gain, start = filled(len(wave), np.float64), filled(B, np.float64), filled(B, np.float64), filled(B, np.int64)
        m = (ptr(masker), ptr(moff), len(recordings), ptr(mof)) if with_maskers else (None, None, 0, None)
        rc = ctx.lib.f2_masker_pick(ctx.handle, ptr(wave), _lib.WAVE_I16, ptr(offsets), B, ptr(snr) if k else None, *m, k, ptr(level), 0, SEED,
                                    ptr(out), ptr(sigma), ptr(gain), ptr(start), _lib.MEM_HOST)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        assert bits(out).tobytes() == want, (k, with_maskers)
        assert (sigma == 0).all() and (gain == 0).all() and (start == 0).all(), (k, with_maskers)


def test_every_error_comes_before_anything_is_written(ctx):
    wave, offsets = mc.ragged_waves()
    recordings, masker_of, snr = mc.SETS["wraps"]
    masker, moff = _lib._pack_rirs(recordings)
    outs = [filled(len(wave), np.float64), filled(B, np.float64), filled(B, np.float64), filled(B, np.int64)]

    def call(snr=np.array(snr, np.float64), masker=masker, moff=moff, r=len(recordings), mof=np.array(masker_of, np.int32), k=K,
             level=np.array(LEVEL_OF, np.int32), first=0):
        return ctx.lib.f2_masker_pick(ctx.handle, ptr(wave), _lib.WAVE_I16, ptr(offsets), B, ptr(snr), ptr(masker), ptr(moff), r, ptr(mof), k,
                                      ptr(level), first, SEED, *[ptr(o) for o in outs], _lib.MEM_HOST)
    bad_level, nan, empty, bad_of = np.array(LEVEL_OF, np.int32), masker.copy(), moff.copy(), np.array(masker_of, np.int32)
    bad_level[4], nan[2], empty[3], bad_of[2] = K + 1, np.nan, empty[2], -1
    for kw, status, word in ((dict(level=bad_level), INV, "utterance 4"), (dict(masker=None), INV, "masker"), (dict(masker=nan), INV, "recording 1: sample 1"),
                             (dict(moff=empty), INV, "recording 2 is empty"), (dict(mof=bad_of), INV, "level 2"), (dict(k=-1), INV, "K=-1"),
                             (dict(snr=None), INV, "snr_db is NULL"), (dict(first=2 ** 32 - 3), UNS, "utterance number"),
                             (dict(r=65), UNS, "65 recordings"), (dict(k=65, level=np.zeros(B, np.int32)), UNS, "65 masker levels")):
        if "k" in kw and kw["k"] == 65:
            kw.update(snr=np.zeros(65), mof=np.zeros(65, np.int32))
        assert call(**kw) == status, list(kw)
        msg = ctx.lib.f2_last_error(ctx.handle).decode()
        assert word in msg, (list(kw), msg)
        assert all((bits(o) == mc.FILL).all() for o in outs), list(kw)
    assert call() == _lib.F2_OK and np.isfinite(outs[0]).all()
