"""Addressing of the spectral row kernels (f2cnn_amd/csrc/f2_spectral.hip, f2_fft13_merged.h): the spectrum phase of
k_spectral_envelope reads the utterance spectrum and the channel table through scalar buffer descriptors (lane byte offset + a scalar
offset per bin), the merged passes 1 + 2 store their sixteen outputs at padded addresses, the row stores go out block by block. One
batch per instantiation at its smallest shapes - k_spectral_envelope<12|13|14, single-block> (uniform rows of at
least 15/16 of the transform), <12|13|14, general> (ragged: the shortest row of the class, odd padding, padding that ends on a
block) and k_spectral_envelope_long (shortest, a middle and the longest row) - with the low-pass off and at 50 Hz, the output
pre-filled with NaN: a bin, an exchange slot or a store block addressed wrongly shows as a NaN left or as an error far above the
bounds. Conventions of tests/test_gpu_spectral_front_padding.py (8 channels, spectral_min_rows=0).
The route takes a row only if its padding holds the peak of the slowest channel's ringing (f2_spectral_supports_len): 256 samples
for a bank that starts at 100 Hz, so the longest row the long-row kernel can serve at all, 65472 samples (64 of padding), is only
routed with a bank whose lowest channel rings shorter. That batch therefore uses eight channels from 1 kHz up (64 samples); the
100 Hz bank runs on the long-row kernel in a batch of its own, up to ITS longest row, 65280 samples."""
import functools

import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters

pytestmark = pytest.mark.gpu
TOL = 1e-5          # per-channel max-norm, relative (north star)
ROUTES = 4e-6       # the project's bound between the spectral and the two-kernel route
C = 8

BATCHES = {
    "<12, single-block> uniform 7935": [7935] * 3,
    "<12, general> ragged": [4097, 7680],
    "<13, single-block> uniform 16000": [16000] * 3,
    "<13, general> ragged": [8193, 15999],
    "<14, single-block> uniform 32511": [32511] * 3,
    "<14, general> ragged": [16385, 30720],
    "long rows": [32769, 40000, 65472],
    "long rows, 100 Hz bank": [32769, 65280],
}
LOW_HZ = {"long rows": 1000}      # lowest centre frequency of the batch's bank (default 100)
SETTINGS = [(False, 0.0), (True, 50.0)]


@functools.lru_cache(maxsize=None)
def coefs(low_hz=100):
    return filters.make_erb_filters(16000, filters.centre_freqs(16000, C, low_hz))


@functools.lru_cache(maxsize=None)
def wave(seed, n):
    w = orc.synth_utterance(seed, n)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(seed, n, lpf, cutoff, low_hz):
    ref = orc.filter_and_envelope(wave(seed, n), coefs(low_hz), lpf, cutoff)
    ref.setflags(write=False)
    return ref


def chan_relerr(a, b):
    return float((np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max())


def fused(ctx, waves, lpf, cutoff, low_hz, **opts):
    offs = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    flat = np.concatenate(waves)
    env = np.full(C * int(offs[-1]), np.nan)
    with ctx.options(spectral_min_rows=0, **opts):
        ctx.filterbank_envelope_fused(flat, _lib.WAVE_I16, offs, coefs(low_hz), len(waves), C, lpf, cutoff, _lib.FFT_F32, env, None, _lib.MEM_HOST)
        routed, flagged = int(ctx.get_option("spectral_routed")), int(ctx.get_option("spectral_flagged"))
    return [env[C * offs[b]:C * offs[b + 1]].reshape(C, -1) for b in range(len(waves))], routed, flagged


@pytest.mark.parametrize("lpf,cutoff", SETTINGS, ids=["lpf off", "50 Hz"])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_every_instantiation_against_oracle_and_two_kernel_route(batch, lpf, cutoff):
    ctx = _lib.default_context()
    lens, low_hz = BATCHES[batch], LOW_HZ.get(batch, 100)
    seeds = [4100 + 10 * list(BATCHES).index(batch) + i for i in range(len(lens))]
    waves = [wave(s, n) for s, n in zip(seeds, lens)]
    got, routed, flagged = fused(ctx, waves, lpf, cutoff, low_hz, spectral=1)
    old, _, _ = fused(ctx, waves, lpf, cutoff, low_hz, spectral=0)
    assert routed == len(lens)
    assert flagged == 0
    for s, n, g, o in zip(seeds, lens, got, old):
        assert not np.isnan(g).any(), n
        ref = reference(s, n, lpf, cutoff, low_hz)
        assert g.shape == ref.shape
        e_ref, e_old = chan_relerr(g, ref), chan_relerr(g, o)
        print(f"{batch} n {n}: against the oracle {e_ref:.2e}, against the two-kernel route {e_old:.2e}")
        assert e_ref <= TOL, n
        assert e_old <= ROUTES, n
