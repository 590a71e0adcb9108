"""f2_input_batch_filtered: an envelope cutoff per utterance between the envelopes and the gather. The one call against the
stateless calls it is made of, on raw bytes: the unfiltered envelopes of the batch (f2_filterbank_envelope_fused with gfb NULL and
lpf = 0, the call f2_input_batch's own envelopes are held against in tests/test_gpu_input_from_wav.py), f2_lowpass_levels on them,
f2_gather_windows on block cutoff_of[b] for utterance b. Without the stage against f2_input_batch_masked; with a noise level per
file and with a mixing matrix per file against the same construction behind f2_noise_pick and in front of f2_gather_windows_mixed;
the errors of the stage, which come before any launch; and the history of the context.

4 channels at 16 kHz, five seeded speech-like utterances of 1500 .. 9000 samples - one too short for a window of radius 5 at step
160, one longer than two 4096-sample segments of the filter kernel - and cutoffs of 5, 50 and 400 Hz, which keep the envelopes
positive."""
import numpy as np
import pytest

import f2cnn_oracle as orc
import speechlike
from f2cnn_amd import _lib

pytestmark = pytest.mark.gpu

C, RADIUS, STEP = 4, 5, 160
R, REACH = 2 * RADIUS + 1, RADIUS * STEP
LENGTHS = (1500, 4097, 9000, 2500, 6001)
B = len(LENGTHS)
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
CUTOFFS = (5.0, 50.0, 400.0)
KC = len(CUTOFFS)
CUTOFF_OF = (1, 0, 2, 3, 1)                    # every cutoff and the unfiltered level
SNR, LEVEL_OF, SEED, FIRST = (20.0, 6.0), (0, 2, 1, 0, 1), 0x1234_5678_9ABC, 3
MIX_OF = (0, 2, 1, 1, 0)
FILL = 0x5A
HOST, DEV = _lib.MEM_HOST, _lib.MEM_DEVICE
I16, F64 = _lib.WAVE_I16, _lib.WAVE_F64


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def ptr(a):
    return None if a is None else a.ctypes.data


def centres():
    rng = np.random.default_rng(11)
    cs = []
    for n in LENGTHS:
        if n < 2 * REACH + 1:
            cs.append(np.zeros(0, np.int64))
            continue
        c = rng.integers(REACH, n - REACH, size=4)
        c[0], c[-1] = REACH, n - 1 - REACH
        cs.append(c.astype(np.int64))
    return cs, np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)


def matrices():
    m = np.random.default_rng(5).random((2, C, C)) + np.eye(C)
    return m / m.sum(axis=2, keepdims=True)


@pytest.fixture(scope="module")
def batch(ctx):
    """waves, filterbank, centres, and the reference of the stage alone: computed once, only read"""
    flat = np.concatenate([speechlike.make(470 + i, n)[0] for i, n in enumerate(LENGTHS)]).astype(np.int16)
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))
    cs, coff = centres()
    want = reference(ctx, flat, I16, coefs, cs, CUTOFF_OF)
    for a in (flat, coefs, coff, want):
        a.setflags(write=False)
    return flat, coefs, cs, coff, want


def levels_of(ctx, wave, dt, coefs):
    """(KC + 1, C * total): f2_lowpass_levels on the unfiltered envelopes of the batch"""
    env = np.empty(C * len(wave))
    ctx.filterbank_envelope_fused(wave, dt, OFFSETS, coefs, B, C, False, 0.0, _lib.FFT_F32, env, None, HOST)
    levels = np.empty((KC + 1, env.size))
    ctx.lowpass_levels(env, OFFSETS, B, C, CUTOFFS, levels, HOST)
    return levels


def reference(ctx, wave, dt, coefs, cs, cutoff_of):
    """f2_gather_windows(normalize = 1) per utterance on its level's block of the sweep"""
    levels = levels_of(ctx, wave, dt, coefs)
    out = []
    for b, n in enumerate(LENGTHS):
        if not len(cs[b]):
            continue
        env_b = np.ascontiguousarray(levels[cutoff_of[b]][C * OFFSETS[b]:C * OFFSETS[b + 1]])
        w = np.full((len(cs[b]), R, C), np.nan, np.float32)
        ctx.gather_windows(env_b, C, n, cs[b], len(cs[b]), RADIUS, STEP, True, w, HOST)
        out.append(w)
    return np.concatenate(out)


def filtered(ctx, batch, wave=None, dt=I16, lpf=0, snr=(), level_of=None, mixes=None, mix_of=None, cutoffs=CUTOFFS, cutoff_of=CUTOFF_OF,
             mem=HOST, call=None):
    flat, coefs, cs, coff, _ = batch
    wave = flat if wave is None else wave
    out = np.full((int(coff[-1]), R, C), np.nan, np.float32)
    args = (OFFSETS, coefs, B, C, bool(lpf), float(lpf), _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP, True, (), None, snr, None,
            level_of, FIRST, SEED, mixes, mix_of, None, None, (), None)
    tail = (cutoffs, cutoff_of) if call is None else ()
    call = call or ctx.input_batch_filtered
    if mem == HOST:
        call(wave, dt, *args, *tail, out, mem)
        return out
    d_in, d_out = ctx.malloc(wave.nbytes), ctx.malloc(out.nbytes)
    try:
        ctx.h2d(d_in, wave)
        ctx.h2d(d_out, out)
        ctx.synchronize()
        call(d_in, dt, *args, *tail, d_out, mem)
        ctx.synchronize()
        ctx.d2h(out, d_out)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    return out


@pytest.mark.parametrize("mem", [HOST, DEV], ids=["host", "device"])
def test_windows_are_the_gather_on_the_utterances_level_of_the_sweep(ctx, batch, mem):
    flat, coefs, cs, coff, want = batch
    got = filtered(ctx, batch, mem=mem)
    assert len(got) == 16 and np.isfinite(got).all()
    assert bits(got).tobytes() == bits(want).tobytes()
    # utterance 3 is unfiltered: its windows are f2_input_batch(lpf = 0)'s, and those of the filtered utterances are not
    plain = np.full_like(got, np.nan)
    ctx.input_batch(flat, I16, OFFSETS, coefs, B, C, False, 0.0, _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP, True, plain, HOST)
    w = [int(coff[b]) for b in range(B + 1)]
    assert bits(got[w[3]:w[4]]).tobytes() == bits(plain[w[3]:w[4]]).tobytes()
    for b in (1, 2, 4):
        assert not np.array_equal(got[w[b]:w[b + 1]], plain[w[b]:w[b + 1]]), b
    everywhere = filtered(ctx, batch, cutoff_of=(KC,) * B, mem=mem)
    assert bits(everywhere).tobytes() == bits(plain).tobytes()


@pytest.mark.parametrize("lpf", [0, 50])
def test_without_the_stage_it_is_input_batch_masked(ctx, batch, lpf):
    want = filtered(ctx, batch, lpf=lpf, snr=SNR, level_of=LEVEL_OF, mixes=matrices(), mix_of=MIX_OF, call=ctx.input_batch_masked)
    for cutoffs, cutoff_of in (((), None), (CUTOFFS, None), ((), CUTOFF_OF)):
        got = filtered(ctx, batch, lpf=lpf, snr=SNR, level_of=LEVEL_OF, mixes=matrices(), mix_of=MIX_OF, cutoffs=cutoffs, cutoff_of=cutoff_of)
        assert bits(got).tobytes() == bits(want).tobytes(), (cutoffs, cutoff_of)


def test_behind_a_noise_level_per_file(ctx, batch):
    flat, coefs, cs, coff, clean = batch
    got = filtered(ctx, batch, snr=SNR, level_of=LEVEL_OF)
    noisy = np.empty(len(flat))
    ctx.noise_pick(flat, I16, OFFSETS, B, SNR, LEVEL_OF, FIRST, SEED, noisy, HOST)
    want = reference(ctx, noisy, F64, coefs, cs, CUTOFF_OF)
    assert bits(got).tobytes() == bits(want).tobytes() and not np.array_equal(got, clean)


def test_in_front_of_a_mixing_matrix_per_file(ctx, batch):
    flat, coefs, cs, coff, sharp = batch
    mix = matrices()
    got = filtered(ctx, batch, mixes=mix, mix_of=MIX_OF)
    env = np.empty(C * len(flat))
    ctx.filterbank_envelope_fused(flat, I16, OFFSETS, coefs, B, C, False, 0.0, _lib.FFT_F32, env, None, HOST)
    picked = np.empty_like(env)
    ctx.lowpass_pick(env, OFFSETS, B, C, CUTOFFS, CUTOFF_OF, picked, HOST)
    want = np.full_like(got, np.nan)
    ctx.gather_windows_mixed(picked, OFFSETS, B, C, coff, np.concatenate(cs), RADIUS, STEP, True, mix, MIX_OF, want, HOST)
    assert bits(got).tobytes() == bits(want).tobytes() and not np.array_equal(got, sharp)


def test_every_stage_at_once(ctx, batch):
    """rooms, maskers, coloured noise, cutoffs and matrices in one call (the most small arrays a call names): host and device memory
    give the same bytes, and the call without cutoffs other ones"""
    from f2cnn_amd.reverb import SyntheticRIR
    flat, coefs, cs, coff, _ = batch
    rng = np.random.default_rng(8)
    rirs = [SyntheticRIR(1.0, t, seed=9, level=l) for l, t in enumerate((7, 1025))]
    firs = [rng.standard_normal(t) / t for t in (5, 300)]
    maskers = [rng.standard_normal(n) * 900.0 for n in (7, 5000)]
    stages = (rirs, (1, 2, 0, 2, 0), SNR, firs, LEVEL_OF, FIRST, SEED, matrices(), MIX_OF, maskers, (0, 1, 1), (10.0, 0.0, 6.0), (3, 0, 2, 1, 2))
    front = (OFFSETS, coefs, B, C, False, 0.0, _lib.FFT_F32, coff, np.concatenate(cs), RADIUS, STEP, True)
    host = np.full((int(coff[-1]), R, C), np.nan, np.float32)
    ctx.input_batch_filtered(flat, I16, *front, *stages, CUTOFFS, CUTOFF_OF, host, HOST)
    assert np.isfinite(host).all()
    dev = np.full_like(host, np.nan)
    d_in, d_out = ctx.malloc(flat.nbytes), ctx.malloc(dev.nbytes)
    try:
        ctx.h2d(d_in, flat)
        ctx.input_batch_filtered(d_in, I16, *front, *stages, CUTOFFS, CUTOFF_OF, d_out, DEV)
        ctx.synchronize()
        ctx.d2h(dev, d_out)
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    assert bits(dev).tobytes() == bits(host).tobytes()
    bare = np.full_like(host, np.nan)
    ctx.input_batch_masked(flat, I16, *front, *stages, bare, HOST)
    w = [int(v) for v in coff]
    assert bits(bare[w[3]:w[4]]).tobytes() == bits(host[w[3]:w[4]]).tobytes() and not np.array_equal(bare[:w[3]], host[:w[3]])


def test_errors_of_the_stage_come_before_any_launch(ctx, batch):
    flat, coefs, cs, coff, want = batch
    cen = np.concatenate(cs)
    out = np.empty((int(coff[-1]), R, C), np.float32)
    bits(out)[...] = FILL

    def call(lpf=0, cut=np.array(CUTOFFS), kc=KC, cof=np.array(CUTOFF_OF, np.int32)):
        return ctx.lib.f2_input_batch_filtered(ctx.handle, ptr(flat), I16, ptr(OFFSETS), ptr(coefs), B, C, lpf, 50.0 if lpf else 0.0,
                                               _lib.FFT_F32, ptr(coff), ptr(cen), RADIUS, STEP, 1, None, None, 0, None, None, None, None, 0,
                                               None, FIRST, SEED, None, 0, None, None, None, None, 0, None, 0, None, ptr(cut), kc, ptr(cof),
                                               ptr(out), HOST)
    bad_of, low_of, nan, inf = np.array(CUTOFF_OF, np.int32), np.array(CUTOFF_OF, np.int32), np.array(CUTOFFS), np.array(CUTOFFS)
    bad_of[2], low_of[4], nan[1], inf[0] = KC + 1, -1, np.nan, np.inf
    INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    for kw, status, words in ((dict(lpf=1), INV, ("cutoff", "lpf")), (dict(cof=bad_of), INV, ("utterance 2",)),
                              (dict(cof=low_of), INV, ("utterance 4",)), (dict(cut=nan), INV, ("cutoff_hz[1]",)),
                              (dict(cut=inf), INV, ("cutoff_hz[0]",)), (dict(cut=np.full(65, 50.0), kc=65), UNS, ("65 cutoffs",)),
                              (dict(kc=-1), INV, ("K=-1",)), (dict(cut=None), INV, ("cutoff_hz is NULL",))):
        assert call(**kw) == status, list(kw)
        said = ctx.lib.f2_last_error(ctx.handle).decode()
        assert all(w in said for w in words), (list(kw), said)
        assert (bits(out) == FILL).all(), list(kw)
    assert call() == _lib.F2_OK and bits(out).tobytes() == bits(want).tobytes()


def test_the_bytes_do_not_depend_on_what_the_context_ran_before(ctx, batch):
    flat, coefs, cs, coff, want = batch
    first = filtered(ctx, batch, snr=SNR, level_of=LEVEL_OF, mixes=matrices(), mix_of=MIX_OF)
    again = filtered(ctx, batch, snr=SNR, level_of=LEVEL_OF, mixes=matrices(), mix_of=MIX_OF)
    assert bits(first).tobytes() == bits(again).tobytes()
    # an unrelated call with other shapes: 7 channels, three short utterances, more cutoffs, no other stage
    n2 = (1761, 3000, 1999)
    off2 = np.concatenate([[0], np.cumsum(n2)]).astype(np.int64)
    w2 = np.concatenate([orc.synth_utterance(90 + i, n) for i, n in enumerate(n2)]).astype(np.int16)
    coefs2 = orc.make_erb_filters(16000, orc.centre_freqs(16000, 7, 100))
    cen2, coff2 = np.array([REACH, REACH + 1, n2[1] - 1 - REACH], np.int64), np.array([0, 1, 3, 3], np.int64)
    other = np.full((3, R, 7), np.nan, np.float32)
    ctx.input_batch_filtered(w2, I16, off2, coefs2, 3, 7, False, 0.0, _lib.FFT_F32, coff2, cen2, RADIUS, STEP, True, (), None, (), None, None,
                             0, 0, None, None, None, None, (), None, (3.0, 30.0, 300.0, 1000.0, 10.0), (4, 3, 0), other, HOST)
    assert np.isfinite(other).all()
    once_more = filtered(ctx, batch, snr=SNR, level_of=LEVEL_OF, mixes=matrices(), mix_of=MIX_OF)
    assert bits(once_more).tobytes() == bits(first).tobytes()
    assert bits(filtered(ctx, batch)).tobytes() == bits(want).tobytes()
