"""The first instructions of a row in the spectral row kernels (f2cnn_amd/csrc/f2_spectral.hip): the row's (utterance, channel) is
decoded from a two-dimensional grid with a reciprocal from the host (the partial last channel group is a launch of its own), the
twiddles of the later passes and the two twiddles of the first pass are loaded in front of the table loads, the Nyquist bin and the
row's digits are loaded once, by every wave, with the row's other scalar loads. What each of these can get wrong, at the smallest
shapes that show it:

    block decode            a wrong decode permutes rows: every (utterance, channel) row is compared on its own, and every row
                            differs. C below, at and above one and two channel groups of 32, 1 and 3 utterances; one ragged batch
                            whose utterances alternate between two length classes (two kernels in the call, ulist[u] != u)
    twiddle fill, pass 0    one batch per instantiation at its smallest shape (256-, 512- and 1024-thread workgroups: threads beyond
                            the table, more than one entry per thread), lengths of tests/test_gpu_spectral_addressing.py
    Nyquist bin             a wave at half the sampling rate plus a little noise, 128-channel bank, the four highest channels
    history                 A, B, A on one context, A's outputs byte for byte (tests/call_history.py)

Conventions of tests/test_gpu_spectral.py: spectral_min_rows=0 forces the route, outputs pre-filled with NaN, every utterance routed
and none flagged, every row within 1e-5 of its maximum of the oracle and within 4e-6 of the two-kernel route."""
import functools

import numpy as np
import pytest

import call_history as ch
import f2cnn_oracle as orc
import test_gpu_spectral_addressing as addressing
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from test_gpu_spectral import TOL, chan_relerr

pytestmark = pytest.mark.gpu
ROUTES = addressing.ROUTES      # 4e-6, the project's bound between the spectral and the two-kernel route


@functools.lru_cache(maxsize=None)
def bank(C, low_hz=100):
    coefs = filters.make_erb_filters(16000, filters.centre_freqs(16000, C, low_hz))
    coefs.setflags(write=False)
    return coefs


@functools.lru_cache(maxsize=None)
def wave(seed, n):
    w = orc.synth_utterance(seed, n)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def reference(seed, n, C, lpf, cutoff):
    ref = orc.filter_and_envelope(wave(seed, n), bank(C), lpf, cutoff)
    ref.setflags(write=False)
    return ref


def fused(ctx, waves, coefs, lpf, cutoff, **opts):
    """[(C, n) envelopes], routed, flagged; the output starts as NaN"""
    C = coefs.shape[0]
    offs = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    env = np.full(C * int(offs[-1]), np.nan)
    with ctx.options(spectral_min_rows=0, **opts):
        ctx.filterbank_envelope_fused(np.concatenate(waves), _lib.WAVE_I16, offs, coefs, len(waves), C, lpf, cutoff, _lib.FFT_F32, env, None,
                                      _lib.MEM_HOST)
        routed, flagged = int(ctx.get_option("spectral_routed")), int(ctx.get_option("spectral_flagged"))
    return [env[C * offs[b]:C * offs[b + 1]].reshape(C, -1) for b in range(len(waves))], routed, flagged


def check_rows(ctx, seeds, lens, C, lpf, cutoff):
    """every (utterance, channel) row of the spectral route against the oracle and against the two-kernel route"""
    waves = [wave(s, n) for s, n in zip(seeds, lens)]
    got, routed, flagged = fused(ctx, waves, bank(C), lpf, cutoff, spectral=1)
    old, _, _ = fused(ctx, waves, bank(C), lpf, cutoff, spectral=0)
    assert routed == len(lens)
    assert flagged == 0
    for s, n, g, o in zip(seeds, lens, got, old):
        assert not np.isnan(g).any(), (n, int(np.isnan(g).sum()))
        ref = reference(s, n, C, lpf, cutoff)
        assert g.shape == ref.shape
        e_ref, e_old = chan_relerr(g, ref), chan_relerr(g, o)       # (the largest over the rows, each relative to its own maximum)
        print(f"C {C} n {n}: against the oracle {e_ref:.2e}, against the two-kernel route {e_old:.2e}")
        assert e_ref <= TOL, (C, n)
        assert e_old <= ROUTES, (C, n)


@pytest.mark.parametrize("nutt", [1, 3])
@pytest.mark.parametrize("C", [1, 8, 31, 32, 33, 40, 65])
def test_block_decode(C, nutt):
    """C = 1, 8, 31: one partial group alone; 32: one full group; 33, 40: a full group and a partial one (two launches); 65: two full
    groups and a group of one channel"""
    check_rows(_lib.default_context(), [5200 + i for i in range(nutt)], [9000] * nutt, C, True, 50.0)


def test_block_decode_two_length_classes_alternating():
    """5000 and 9000 samples in turn: each length class's kernel gets utterances 0, 2 / 1, 3 of the batch as its 0, 1"""
    check_rows(_lib.default_context(), [5300, 5301, 5302, 5303], [5000, 9000, 5000, 9000], 40, True, 50.0)


SMALLEST = {name: (lens[:1] if "uniform" in name else lens) for name, lens in addressing.BATCHES.items() if name != "long rows, 100 Hz bank"}
SMALLEST["long rows"] = [32769]


@pytest.mark.parametrize("lpf,cutoff", addressing.SETTINGS, ids=["lpf off", "50 Hz"])
@pytest.mark.parametrize("batch", list(SMALLEST))
def test_twiddles_of_every_instantiation(batch, lpf, cutoff):
    """8 channels (tests/test_gpu_spectral_addressing.py: its bank, waves and references)"""
    ctx = _lib.default_context()
    lens = SMALLEST[batch]
    seeds = [4100 + 10 * list(addressing.BATCHES).index(batch) + i for i in range(len(lens))]
    waves = [addressing.wave(s, n) for s, n in zip(seeds, lens)]
    got, routed, flagged = addressing.fused(ctx, waves, lpf, cutoff, 100, spectral=1)
    old, _, _ = addressing.fused(ctx, waves, lpf, cutoff, 100, spectral=0)
    assert routed == len(lens)
    assert flagged == 0
    for s, n, g, o in zip(seeds, lens, got, old):
        assert not np.isnan(g).any(), n
        ref = addressing.reference(s, n, lpf, cutoff, 100)
        assert g.shape == ref.shape
        e_ref, e_old = chan_relerr(g, ref), chan_relerr(g, o)
        print(f"{batch} n {n}: against the oracle {e_ref:.2e}, against the two-kernel route {e_old:.2e}")
        assert e_ref <= TOL, n
        assert e_old <= ROUTES, n


@pytest.mark.parametrize("n", [9000, 16000])
def test_nyquist_bin(n):
    """A (-1)^t plus noise of a fortieth of A: the four highest channels of the 128-channel bank carry what bin M/2 holds. (9000
    samples: <13, general>; 16000: <13, single-block>, the rows of the benchmark.)"""
    ctx = _lib.default_context()
    C = 128
    cfs = np.asarray(filters.centre_freqs(16000, C, 100))
    top = np.sort(np.argsort(cfs)[-4:])
    rng = np.random.default_rng(5400 + n)
    w = np.round(8000.0 * (1 - 2 * (np.arange(n) & 1)) + 200.0 * rng.standard_normal(n)).astype(np.int16)
    for lpf, cutoff in addressing.SETTINGS:
        (got,), routed, flagged = fused(ctx, [w], bank(C), lpf, cutoff, spectral=1)
        (old,), _, _ = fused(ctx, [w], bank(C), lpf, cutoff, spectral=0)
        assert routed == 1
        assert flagged == 0
        assert not np.isnan(got).any()
        ref = orc.filter_and_envelope(w, bank(C)[top], lpf, cutoff)
        e_ref, e_old = chan_relerr(got[top], ref), chan_relerr(got[top], old[top])
        print(f"n {n} lpf {lpf}: channels {top.tolist()} against the oracle {e_ref:.2e}, against the two-kernel route {e_old:.2e}")
        assert e_ref <= TOL
        assert e_old <= ROUTES


def test_history_a_b_a():
    """the 40-channel batch of the decode test (two launches of the row kernel), a batch of another length class and bank, the first
    again: each call byte for byte what it gives on a context of its own"""
    a = ch.fused((9000, 9000, 9000), C=40, routed=3, flagged=0, seed=3)
    b = ch.fused((5000,), C=8, tab="erb1000", lpf=False, routed=1, flagged=0, seed=4)
    with ch.context() as ctx:
        ch.replay(ctx, [a, b, a])
