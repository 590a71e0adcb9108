"""k_spectral_envelope<13, .> with one LDS pad per 32 points, the first-pass butterflies dealt by parity and single 8-byte reads
in the exchanges (f2cnn_amd/csrc/f2_fft13_merged.h: Pad32, pass0_deal; the index maps alone: tests/test_ks_lds_layout.py). The deal
moves which bins a thread loads, which phase factor and first-pass twiddles it takes and where it stores; a bin, a twiddle or an
exchange slot taken by the thread's own number instead shows as a NaN left in the pre-filled output or as an error far above the
bounds. Batches: <13, single-block> at 16000 samples and at the ends of its class (15360, 16128), <13, general> ragged (8193, 9000,
15359), one 128-channel batch whose wave carries a tone at half the sampling rate (thread 0 forms the Nyquist bin after the deal),
and one batch per other instantiation (<12>, <14>, long rows; shapes of tests/test_gpu_spectral_addressing.py), whose layout is
the one before. Low-pass off and at 50 Hz, int16 waves, spectral_min_rows=0. Bars as everywhere: 1e-5 per channel against the
oracle, 4e-6 against the two-kernel route; every utterance routed, none flagged."""
import functools

import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters

pytestmark = pytest.mark.gpu
TOL = 1e-5          # per-channel max-norm, relative (north star)
ROUTES = 4e-6       # the project's bound between the spectral and the two-kernel route

# name: (channels, lengths, wave kind)
BATCHES = {
    "<13, single-block> 2 x 16000": (8, [16000, 16000], "noise"),
    "<13, single-block> ends of the class": (8, [15360, 16128], "noise"),
    "<13, general> ragged": (8, [8193, 9000, 15359], "noise"),
    "<13, single-block> 128 channels, tone at half the sampling rate": (128, [16000], "nyquist"),
    "<12, single-block> uniform 7935": (8, [7935] * 3, "noise"),
    "<14, single-block> uniform 32511": (8, [32511] * 3, "noise"),
    "long rows, 100 Hz bank": (8, [32769, 65280], "noise"),
}
SETTINGS = [(False, 0.0), (True, 50.0)]


@functools.lru_cache(maxsize=None)
def coefs(C):
    return filters.make_erb_filters(16000, filters.centre_freqs(16000, C, 100))


@functools.lru_cache(maxsize=None)
def wave(seed, n, kind):
    if kind == "nyquist":
        # x[i] = 6000 (-1)^i on top of noise: all of the tone's energy sits in bin H of the 16384-point spectrum
        w = orc.synth_utterance(seed, n, 1500.0).astype(np.int32) + 6000 * (1 - 2 * (np.arange(n) & 1))
        w = np.clip(w, -32768, 32767).astype(np.int16)
    else:
        w = orc.synth_utterance(seed, n)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(seed, n, kind, C, lpf, cutoff):
    ref = orc.filter_and_envelope(wave(seed, n, kind), coefs(C), lpf, cutoff)
    ref.setflags(write=False)
    return ref


def chan_relerr(a, b):
    return float((np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max())


def fused(ctx, waves, C, lpf, cutoff, **opts):
    offs = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    flat = np.concatenate(waves)
    env = np.full(C * int(offs[-1]), np.nan)
    with ctx.options(spectral_min_rows=0, **opts):
        ctx.filterbank_envelope_fused(flat, _lib.WAVE_I16, offs, coefs(C), len(waves), C, lpf, cutoff, _lib.FFT_F32, env, None, _lib.MEM_HOST)
        routed, flagged = int(ctx.get_option("spectral_routed")), int(ctx.get_option("spectral_flagged"))
    return [env[C * offs[b]:C * offs[b + 1]].reshape(C, -1) for b in range(len(waves))], routed, flagged


@pytest.mark.parametrize("lpf,cutoff", SETTINGS, ids=["lpf off", "50 Hz"])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_rows_against_oracle_and_two_kernel_route(batch, lpf, cutoff):
    ctx = _lib.default_context()
    C, lens, kind = BATCHES[batch]
    seeds = [4300 + 10 * list(BATCHES).index(batch) + i for i in range(len(lens))]
    waves = [wave(s, n, kind) for s, n in zip(seeds, lens)]
    got, routed, flagged = fused(ctx, waves, C, lpf, cutoff, spectral=1)
    old, _, _ = fused(ctx, waves, C, lpf, cutoff, spectral=0)
    assert routed == len(lens)
    assert flagged == 0
    for s, n, g, o in zip(seeds, lens, got, old):
        assert not np.isnan(g).any(), n
        ref = reference(s, n, kind, C, lpf, cutoff)
        assert g.shape == ref.shape
        e_ref, e_old = chan_relerr(g, ref), chan_relerr(g, o)
        print(f"{batch} n {n}: against the oracle {e_ref:.2e}, against the two-kernel route {e_old:.2e}")
        assert e_ref <= TOL, n
        assert e_old <= ROUTES, n
