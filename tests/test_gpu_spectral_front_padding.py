"""Rows of up to 32768 samples padded IN FRONT in the spectral kernels (f2cnn_amd/csrc/f2_spectral.hip: k_utterance_spectrum<FRONT>,
k_spectral_envelope): transform sample i is row sample i - np, np = M - n. Lengths where np is odd (the pair that straddles the
row's start stores its second element only), where the padding ends on a block of the transform's register layout (M / 16
samples), at the threshold of the single-block instantiation (every row of the launch >= 15 M / 16: np = M / 16 exactly is a first
block made of padding only) and at the shortest padding the route accepts (256 samples); the utterance spectrum decimated by two
(16385..32768 samples, odd and even np); LPF off, 50 Hz and 5 Hz; int16 and float64 waves; the accuracy guard on a late click."""
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
    "ragged 8192": [4097, 4098, 7679, 7680, 7681, 7935, 7936],
    "ragged 16384": [8193, 15359, 15360, 15999, 16000, 16127, 16128],
    "ragged 32768": [16385, 20001, 30719, 30720, 32511, 32512],
    "uniform 7680": [7680] * 3,
    "uniform 7935": [7935] * 3,
    "uniform 15999": [15999] * 3,
    "uniform 16000": [16000] * 3,
    "uniform 32511": [32511] * 3,
}
# (LPF, cutoff, float64 waves): every batch with int16 waves at the three low-pass settings, and once with float64 waves
SETTINGS = [(False, 0.0, False), (True, 50.0, False), (True, 5.0, False), (True, 50.0, True)]


@functools.lru_cache(maxsize=None)
def coefs():
    return filters.make_erb_filters(16000, filters.centre_freqs(16000, C, 100))


@functools.lru_cache(maxsize=None)
def wave(seed, n, f64):
    w = orc.synth_utterance(seed, n)
    if f64:     # (not integers: nothing of the int16 path's exactness helps)
        w = w.astype(np.float64) + np.random.default_rng(seed + 77).standard_normal(n)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(seed, n, f64, lpf, cutoff):
    ref = orc.filter_and_envelope(wave(seed, n, f64), coefs(), lpf, cutoff)
    ref.setflags(write=False)
    return ref


def chan_relerr(a, b):
    return float((np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max())


def fused(ctx, waves, lpf, cutoff, **opts):
    offs = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    flat = np.concatenate(waves)
    dtype = _lib.WAVE_I16 if flat.dtype == np.int16 else _lib.WAVE_F64
    env = np.full(C * int(offs[-1]), np.nan)
    with ctx.options(spectral_min_rows=0, **opts):
        ctx.filterbank_envelope_fused(flat, dtype, offs, coefs(), len(waves), C, lpf, cutoff, _lib.FFT_F32, env, None, _lib.MEM_HOST)
        routed, flagged = int(ctx.get_option("spectral_routed")), int(ctx.get_option("spectral_flagged"))
    return [env[C * offs[b]:C * offs[b + 1]].reshape(C, -1) for b in range(len(waves))], routed, flagged


@pytest.mark.parametrize("lpf,cutoff,f64", SETTINGS, ids=["lpf off", "50 Hz", "5 Hz", "50 Hz float64"])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_front_padded_rows_against_oracle_and_two_kernel_route(batch, lpf, cutoff, f64):
    ctx = _lib.default_context()
    lens = BATCHES[batch]
    seeds = [3000 + 10 * list(BATCHES).index(batch) + i for i in range(len(lens))]
    waves = [wave(s, n, f64) for s, n in zip(seeds, lens)]
    got, routed, flagged = fused(ctx, waves, lpf, cutoff, spectral=1)
    old, _, _ = fused(ctx, waves, lpf, cutoff, spectral=0)
    assert routed == len(lens)
    assert flagged == 0
    for s, n, g, o in zip(seeds, lens, got, old):
        assert not np.isnan(g).any(), n          # (an odd row's first sample is stored by a pair of its own kind)
        ref = reference(s, n, f64, lpf, cutoff)
        assert g.shape == ref.shape
        e_ref, e_old = chan_relerr(g, ref), chan_relerr(g, o)
        print(f"{batch} n {n}: against the oracle {e_ref:.2e}, against the two-kernel route {e_old:.2e}")
        assert e_ref <= TOL, n
        assert e_old <= ROUTES, n


@pytest.mark.parametrize("lpf", [False, True], ids=["lpf off", "50 Hz"])
@pytest.mark.parametrize("lens", [[15999] * 3, [12000, 15999, 9000]], ids=["uniform 15999", "ragged"])
def test_late_click_is_still_flagged(lens, lpf):
    """An impulse 10 samples before the end of a row: its ringing, cut at the end of the transform, is what the low channels'
    float32 terms are rounded against. The padding residual - now read in front of the row - must still flag the utterance; the
    two-kernel route recomputes it inside the same call."""
    ctx = _lib.default_context()
    click = np.zeros(15999, np.int16)
    click[15999 - 10] = 32767
    waves = [wave(3200 + i, n, False) if i != 1 else click for i, n in enumerate(lens)]
    got, routed, flagged = fused(ctx, waves, lpf, 50.0, spectral=1)
    assert routed == len(lens)
    assert flagged >= 1
    for w, g in zip(waves, got):
        assert not np.isnan(g).any()
        assert chan_relerr(g, orc.filter_and_envelope(w, coefs(), lpf, 50.0)) <= TOL, len(w)
