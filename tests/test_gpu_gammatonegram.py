"""Gammatonegram pictures (f2_envelope_picture, f2_gammatonegram_batch, `plot gtg`): pooling and range against NumPy / math.fsum,
levels against the LogNorm formula on the device's own pooled values, the wave call against its parts and the oracle, placement
between guard bands, argument errors, and the command's PNG. Shapes are the smallest at which each thing can go wrong."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

import f2cnn_oracle as orc
import speechlike
from devmem import Arena
from f2cnn_amd import _lib, cli
from f2cnn_amd.scripts.plotting import PlottingProcessing as pp
from test_gtg_host import decode_png

pytestmark = pytest.mark.gpu

C5 = 5
LENGTHS = (1000, 257, 0, 4099, 40, 20000)       # C * offsets[b] + c * n_b is odd for some rows; an empty utterance
WIDTHS = (1, 7, 64, 300)                         # 4099 into 1: bins beyond a wave's stride; 40 into 64: m < W; 20000 into 300: many workgroups
SPANS = {"whole": None, "inner": (3, 997), "empty": (100, 100)}     # of the first utterance; the others keep [0, n_b)
MEMS = (_lib.MEM_HOST, _lib.MEM_DEVICE)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def spans_of(lengths, first):
    if first is None:
        return None
    s = np.array([[0, n] for n in lengths], np.int64)
    s[0] = first
    return s


@pytest.fixture(scope="module")
def crafted():
    """the ragged (C5, n_b) float64 blocks, log-normal: exp(3 * normal), seeded"""
    rng = np.random.default_rng(1600)
    return np.concatenate([np.exp(3.0 * rng.standard_normal((C5, n))).reshape(-1) for n in LENGTHS])


def picture(ctx, env, offs, C, spans, W, pool, mem, want=("pooled", "levels", "range")):
    """f2_envelope_picture in `mem`; outputs pre-filled so that an unwritten pixel shows"""
    B = len(offs) - 1
    pooled = np.full((B, C, W), -7.0) if "pooled" in want else None
    levels = np.full((B, C, W), 0xA5, np.uint8) if "levels" in want else None
    rng_out = np.full((B, 2), -7.0) if "range" in want else None
    if mem == _lib.MEM_HOST:
        ctx.envelope_picture(env, offs, B, C, spans, W, pool, pooled, levels, mem, range_out=rng_out)
        return pooled, levels, rng_out
    d_env, d_pooled, d_levels = ctx.malloc(max(env.nbytes, 8)), ctx.malloc(8 * B * C * W), ctx.malloc(B * C * W)
    try:
        ctx.h2d(d_env, env)
        if pooled is not None:
            ctx.h2d(d_pooled, pooled)
        if levels is not None:
            ctx.h2d(d_levels, levels)
        ctx.envelope_picture(d_env, offs, B, C, spans, W, pool, d_pooled if pooled is not None else None,
                             d_levels if levels is not None else None, mem, range_out=rng_out)
        if pooled is not None:
            ctx.d2h(pooled, d_pooled)
        if levels is not None:
            ctx.d2h(levels, d_levels)
    finally:
        for p in (d_env, d_pooled, d_levels):
            ctx.free(p)
    return pooled, levels, rng_out


_referee = {}


def referee_pooled(env, lengths, C, spans, W, pool, key):
    """fsum / count or the maximum of every bin of the definition, computed once per case"""
    if key not in _referee:
        offs = offsets_of(lengths)
        out = np.zeros((len(lengths), C, W))
        for b, n in enumerate(lengths):
            s, e = (0, n) if spans is None else (int(spans[b, 0]), int(spans[b, 1]))
            if e == s:
                continue
            lo, hi = pp.column_edges(e - s, W, s)
            block = env[C * offs[b]:C * offs[b + 1]].reshape(C, n)
            for c in range(C):
                for x in range(W):
                    seg = block[c, lo[x]:hi[x]]
                    out[b, c, x] = seg.max() if pool else math.fsum(seg.tolist()) / len(seg)
        _referee[key] = out
    return _referee[key]


def positive_range(picture_b):
    pos = picture_b[picture_b > 0]
    return (pos.min(), pos.max()) if pos.size else (0.0, 0.0)


def referee_levels(pooled, rng_pair):
    """(levels, distance of 254 t + 0.5 from the nearest integer) for one picture, LogNorm over (vmin, vmax)"""
    vmin, vmax = rng_pair
    lev = np.zeros(pooled.shape, np.int64)
    dist = np.ones(pooled.shape)
    pos = pooled > 0
    if pos.any():
        t = np.zeros(pos.sum()) if vmax == vmin else (np.log(pooled[pos]) - np.log(vmin)) / (np.log(vmax) - np.log(vmin))
        val = 254.0 * t + 0.5
        lev[pos] = 1 + np.floor(val).astype(np.int64)
        dist[pos] = np.abs(val - np.rint(val))
    return lev, dist


def check_levels(levels, pooled, rng_out):
    for b in range(pooled.shape[0]):
        want, dist = referee_levels(pooled[b], tuple(rng_out[b]))
        got = levels[b].astype(np.int64)
        assert np.abs(got - want).max() <= 1
        clear = dist > 1e-9
        assert np.array_equal(got[clear], want[clear])
        assert (~clear).sum() <= 0.01 * clear.size


@pytest.mark.parametrize("span", sorted(SPANS))
@pytest.mark.parametrize("pool", (0, 1))
@pytest.mark.parametrize("W", WIDTHS)
def test_pool_range_and_levels_on_crafted_matrices(ctx, crafted, W, pool, span):
    offs, spans = offsets_of(LENGTHS), spans_of(LENGTHS, SPANS[span])
    want = referee_pooled(crafted, LENGTHS, C5, spans, W, pool, (W, pool, span))
    results = [picture(ctx, crafted, offs, C5, spans, W, pool, mem) for mem in MEMS]
    for pooled, levels, rng_out in results:
        if pool:
            assert np.array_equal(pooled.view(np.uint64), want.view(np.uint64))
        else:
            # a sum of m <= 4099 non-negative doubles in any order is within (m - 1) 2^-53 = 4.6e-13 of the exact one
            err = np.abs(pooled - want) / np.where(want > 0, want, 1.0)
            print("W", W, span, "mean: max relative error", err.max())
            assert err.max() <= 1e-12
        for b in range(len(LENGTHS)):
            assert tuple(rng_out[b]) == positive_range(pooled[b])          # bit for bit of the returned pooled
        assert tuple(rng_out[2]) == (0.0, 0.0) and not pooled[2].any() and not levels[2].any()      # the empty utterance
        if span == "empty":
            assert tuple(rng_out[0]) == (0.0, 0.0) and not pooled[0].any() and not levels[0].any()
        check_levels(levels, pooled, rng_out)
    # the same bits in both memory spaces, and on a second call
    again = picture(ctx, crafted, offs, C5, spans, W, pool, _lib.MEM_HOST)
    for a, b_, c_ in zip(results[0], results[1], again):
        assert np.array_equal(a.view(np.uint8), b_.view(np.uint8)) and np.array_equal(a.view(np.uint8), c_.view(np.uint8))


def test_outputs_are_optional(ctx, crafted):
    offs = offsets_of(LENGTHS)
    full = picture(ctx, crafted, offs, C5, None, 64, 0, _lib.MEM_HOST)
    for mem in MEMS:
        for want in (("pooled",), ("levels",), ("range",), ("levels", "range")):
            got = picture(ctx, crafted, offs, C5, None, 64, 0, mem, want=want)
            for name, g, f in zip(("pooled", "levels", "range"), got, full):
                assert (g is None) == (name not in want)
                if g is not None:
                    assert np.array_equal(g.view(np.uint8), f.view(np.uint8)), (mem, want, name)
        assert picture(ctx, crafted, offs, C5, None, 64, 0, mem, want=()) == (None, None, None)
    ctx.envelope_picture(None, np.zeros(1, np.int64), 0, C5, None, 64, 0, None, None, _lib.MEM_HOST)      # B == 0


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("pool", (0, 1))
def test_special_pictures(ctx, pool, mem):
    C, n = 3, 50
    offs = offsets_of((n, n, n))
    env = np.zeros((3, C, n))
    env[1] = 0.37                                                     # one constant positive value
    base = np.exp(3.0 * np.random.default_rng(3).standard_normal((C, n)))
    env[2] = base
    env[2, 0, 4], env[2, 1, 7], env[2, 1, 8], env[2, 2, 49] = 0.0, -2.5, np.nan, -0.0
    odd = np.zeros((C, n), bool)
    odd[0, 4] = odd[1, 7] = odd[1, 8] = odd[2, 49] = True
    pooled, levels, rng_out = picture(ctx, env.reshape(-1), offs, C, None, n, pool, mem)      # one sample per column
    assert not pooled[0].any() and not levels[0].any() and tuple(rng_out[0]) == (0.0, 0.0)
    assert (levels[1] == 1).all() and tuple(rng_out[1]) == (0.37, 0.37) and (pooled[1] == 0.37).all()
    assert np.isnan(pooled[2, 1, 8]) and np.array_equal(pooled[2][~odd], base[~odd]) and pooled[2, 1, 7] == -2.5
    assert (levels[2][odd] == 0).all() and (levels[2][~odd] >= 1).all()
    assert tuple(rng_out[2]) == (base[~odd].min(), base[~odd].max())
    assert levels[2][~odd].min() == 1 and levels[2][~odd].max() == 255
    check_levels(levels, np.where(np.isnan(pooled), -1.0, pooled), rng_out)
    # a NaN sample inside a longer bin makes that pixel NaN, in both modes, and leaves the others alone
    wide, _, rng_w = picture(ctx, env.reshape(-1), offs, C, None, 5, pool, mem)
    assert np.isnan(wide[2, 1, 0]) and np.isfinite(np.delete(wide[2].reshape(-1), 5)).all()
    assert tuple(rng_w[2]) == positive_range(np.where(np.isnan(wide[2]), 0.0, wide[2]))


# ---- the wave call ----
C8 = 8
WAVE_LENGTHS = (3000, 5001, 16000)


@pytest.fixture(scope="module")
def waves():
    return [speechlike.make(40 + i, n, family=speechlike.ORDINARY[i])[0] for i, n in enumerate(WAVE_LENGTHS)]


@pytest.fixture(scope="module")
def coefs8():
    return orc.make_erb_filters(16000, orc.centre_freqs(16000, C8, 100))


def gammatonegram(ctx, flat, offs, coefs, lpf, W, pool, mem, spans=None):
    B = len(offs) - 1
    pooled, levels, rng_out = np.full((B, C8, W), -7.0), np.full((B, C8, W), 0xA5, np.uint8), np.full((B, 2), -7.0)
    args = (_lib.WAVE_I16, offs, coefs, B, C8, bool(lpf), float(lpf), _lib.FFT_F32, spans, W, pool)
    if mem == _lib.MEM_HOST:
        ctx.gammatonegram_batch(flat, *args, pooled, levels, mem, range_out=rng_out)
        return pooled, levels, rng_out
    d_wave, d_pooled, d_levels = ctx.malloc(flat.nbytes), ctx.malloc(pooled.nbytes), ctx.malloc(levels.nbytes)
    try:
        ctx.h2d(d_wave, flat)
        ctx.h2d(d_pooled, pooled)
        ctx.h2d(d_levels, levels)
        ctx.gammatonegram_batch(d_wave, *args, d_pooled, d_levels, mem, range_out=rng_out)
        ctx.d2h(pooled, d_pooled)
        ctx.d2h(levels, d_levels)
    finally:
        for p in (d_wave, d_pooled, d_levels):
            ctx.free(p)
    return pooled, levels, rng_out


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("lpf", (0, 50))
def test_gammatonegram_is_its_parts(ctx, waves, coefs8, lpf, mem):
    offs, flat = offsets_of(WAVE_LENGTHS), np.concatenate(waves)
    env = np.empty(C8 * int(offs[-1]))
    ctx.filterbank_envelope_fused(flat, _lib.WAVE_I16, offs, coefs8, 3, C8, bool(lpf), float(lpf), _lib.FFT_F32, env, None, _lib.MEM_HOST)
    for pool, W, spans in ((0, 300, None), (1, 64, np.array([[5, 2999], [0, 5001], [16000, 16000]], np.int64))):
        want = picture(ctx, env, offs, C8, spans, W, pool, mem)
        got = gammatonegram(ctx, flat, offs, coefs8, lpf, W, pool, mem, spans)
        twice = gammatonegram(ctx, flat, offs, coefs8, lpf, W, pool, mem, spans)
        for w, g, t in zip(want, got, twice):
            assert np.array_equal(w.view(np.uint8), g.view(np.uint8)) and np.array_equal(g.view(np.uint8), t.view(np.uint8))
        assert (got[2][:2, 0] > 0).all()


@pytest.mark.parametrize("lpf", (0, 50))
def test_gammatonegram_against_the_oracle(ctx, waves, coefs8, lpf):
    offs, flat = offsets_of(WAVE_LENGTHS), np.concatenate(waves)
    W = 300
    for pool in (0, 1):
        pooled, _, _ = gammatonegram(ctx, flat, offs, coefs8, lpf, W, pool, _lib.MEM_HOST)
        for b, wave in enumerate(waves):
            env = orc.filter_and_envelope(wave, coefs8, LPF=bool(lpf), CUTOFF=lpf or 100)
            lo, hi = pp.column_edges(len(wave), W)
            ref = np.array([[env[c, lo[x]:hi[x]].max() if pool else env[c, lo[x]:hi[x]].mean() for x in range(W)] for c in range(C8)])
            err = (np.abs(pooled[b] - ref).max(axis=1) / env.max(axis=1)).max()
            print("lpf", lpf, "pool", pool, "utterance", b, "per-channel error", err)
            assert err <= 1e-5      # the project's envelope bound: mean and maximum pooling cannot widen it


def test_every_device_buffer_misaligned_between_guard_bands(ctx, crafted, waves, coefs8):
    W = 64
    offs = offsets_of(LENGTHS)
    B = len(LENGTHS)
    with Arena(ctx) as arena:
        arena.region("env", np.float64, crafted.size, misalign=1, role="in")
        arena.region("pooled", np.float64, B * C5 * W, misalign=1, role="out")
        arena.region("levels", np.uint8, B * C5 * W, misalign=1, role="out")
        arena.upload("env", crafted)
        for pool in (0, 1):
            want = picture(ctx, crafted, offs, C5, None, W, pool, _lib.MEM_HOST)
            rng_out = ctx.envelope_picture(arena.ptr("env"), offs, B, C5, None, W, pool, arena.ptr("pooled"), arena.ptr("levels"),
                                           _lib.MEM_DEVICE)
            arena.check()
            assert arena.unwritten("pooled") == 0
            assert np.array_equal(arena.download("pooled").view(np.uint64), want[0].reshape(-1).view(np.uint64))
            assert np.array_equal(arena.download("levels"), want[1].reshape(-1)) and np.array_equal(rng_out, want[2])
    woffs, flat = offsets_of(WAVE_LENGTHS), np.concatenate(waves)
    with Arena(ctx) as arena:
        arena.region("wave", np.int16, flat.size, misalign=1, role="in")
        arena.region("pooled", np.float64, 3 * C8 * W, misalign=1, role="out")
        arena.region("levels", np.uint8, 3 * C8 * W, misalign=1, role="out")
        arena.upload("wave", flat)
        want = gammatonegram(ctx, flat, woffs, coefs8, 50, W, 0, _lib.MEM_HOST)
        rng_out = ctx.gammatonegram_batch(arena.ptr("wave"), _lib.WAVE_I16, woffs, coefs8, 3, C8, True, 50.0, _lib.FFT_F32, None, W, 0,
                                          arena.ptr("pooled"), arena.ptr("levels"), _lib.MEM_DEVICE)
        arena.check()
        assert arena.unwritten("pooled") == 0
        assert np.array_equal(arena.download("pooled").view(np.uint64), want[0].reshape(-1).view(np.uint64))
        assert np.array_equal(arena.download("levels"), want[1].reshape(-1)) and np.array_equal(rng_out, want[2])


def test_argument_errors_leave_the_outputs_alone(ctx, crafted, waves, coefs8):
    lib, h = ctx.lib, ctx.handle
    INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    B, W = len(LENGTHS), 16
    offs = offsets_of(LENGTHS)
    pooled, levels, rng_out = np.full((B, C5, W), -7.0), np.full((B, C5, W), 0xA5, np.uint8), np.full((B, 2), -7.0)
    p = lambda a: None if a is None else a.ctypes.data
    good = dict(ctx=h, env=crafted, offsets=offs, B=B, C=C5, spans=None, width=W, pool=0, mem=_lib.MEM_HOST)

    def call(**over):
        a = dict(good, **over)
        return lib.f2_envelope_picture(a["ctx"], p(a["env"]), p(a["offsets"]), a["B"], a["C"], p(a["spans"]), a["width"], a["pool"],
                                       p(pooled), p(levels), p(rng_out), a["mem"])

    def bad_span(s, e, b=3):
        sp = np.array([[0, n] for n in LENGTHS], np.int64)
        sp[b] = (s, e)
        return sp

    down = offs.copy()
    down[2] = down[1] - 1
    cases = [("null ctx", dict(ctx=None), INV), ("null offsets", dict(offsets=None), INV), ("null env", dict(env=None), INV),
             ("mem_space 2", dict(mem=_lib.MEM_HOST_ASYNC), INV), ("mem_space 7", dict(mem=7), INV), ("B < 0", dict(B=-1), INV),
             ("C == 0", dict(C=0), INV), ("C < 0", dict(C=-3), INV), ("width 0", dict(width=0), INV), ("width < 0", dict(width=-5), INV),
             ("pool 2", dict(pool=2), INV), ("pool -1", dict(pool=-1), INV), ("offsets[0] != 0", dict(offsets=offs + 1), INV),
             ("decreasing offsets", dict(offsets=down), INV), ("span s < 0", dict(spans=bad_span(-1, 10)), INV),
             ("span e < s", dict(spans=bad_span(10, 9)), INV), ("span e > n", dict(spans=bad_span(0, 4100)), INV),
             ("width 65537", dict(width=65537), UNS)]
    for name, over, code in cases:
        assert call(**over) == code, name
        assert (pooled == -7.0).all() and (levels == 0xA5).all() and (rng_out == -7.0).all(), name
    assert call(spans=bad_span(0, 4100)) == INV and "utterance 3" in lib.f2_last_error(h).decode()
    assert call(width=65536, B=0) == _lib.F2_OK and call(B=0) == _lib.F2_OK and (pooled == -7.0).all()

    # the wave call: the same checks, and everything f2_check_dsp rejects
    woffs, flat = offsets_of(WAVE_LENGTHS), np.concatenate(waves)
    pooled, levels, rng_out = np.full((3, C8, W), -7.0), np.full((3, C8, W), 0xA5, np.uint8), np.full((3, 2), -7.0)
    goodw = dict(ctx=h, wave=flat, dtype=_lib.WAVE_I16, offsets=woffs, coefs=coefs8, B=3, C=C8, lpf=0, cutoff=0.0, fft=_lib.FFT_F32,
                 spans=None, width=W, pool=0, mem=_lib.MEM_HOST)

    def callw(**over):
        a = dict(goodw, **over)
        return lib.f2_gammatonegram_batch(a["ctx"], p(a["wave"]), a["dtype"], p(a["offsets"]), p(a["coefs"]), a["B"], a["C"], a["lpf"],
                                          ctypes.c_double(a["cutoff"]), a["fft"], p(a["spans"]), a["width"], a["pool"], p(pooled),
                                          p(levels), p(rng_out), a["mem"])

    wspan = np.array([[0, 3000], [0, 5002], [0, 16000]], np.int64)
    casesw = [("null ctx", dict(ctx=None), INV), ("null offsets", dict(offsets=None), INV), ("null wave", dict(wave=None), INV),
              ("null coefs", dict(coefs=None), INV), ("mem_space 2", dict(mem=_lib.MEM_HOST_ASYNC), INV), ("B < 0", dict(B=-1), INV),
              ("C == 0", dict(C=0), INV), ("width 0", dict(width=0), INV), ("pool 3", dict(pool=3), INV),
              ("offsets[0] != 0", dict(offsets=woffs + 1), INV), ("span e > n", dict(spans=wspan), INV),
              ("wave_dtype 5", dict(dtype=5), INV), ("fft_precision 2", dict(fft=2), INV), ("cutoff 0", dict(lpf=1, cutoff=0.0), INV),
              ("cutoff 8000", dict(lpf=1, cutoff=8000.0), INV), ("width 65537", dict(width=65537), UNS)]
    for name, over, code in casesw:
        assert callw(**over) == code, name
        assert (pooled == -7.0).all() and (levels == 0xA5).all() and (rng_out == -7.0).all(), name
    assert callw(spans=wspan) == INV and "utterance 1" in lib.f2_last_error(h).decode()
    assert callw(B=0) == _lib.F2_OK and (pooled == -7.0).all()
    assert callw() == _lib.F2_OK and (pooled != -7.0).all()          # (the good call is good)


def test_plot_envelope_spectrogram_is_the_repeated_levels(ctx):
    n, W = 500, 64
    cf = orc.centre_freqs(16000, C8, 100)
    env = np.exp(3.0 * np.random.default_rng(8).standard_normal((C8, n)))
    height, ratios = pp.GetNewHeightERB(env, cf)
    for pool, (start, end) in (("mean", (0, None)), ("max", (5, 400))):
        image = pp.PlotEnvelopeSpectrogram(env, cf, start=start, end=end, width=W, pool=pool, ctx=ctx)
        span = np.array([[start, n if end is None else end]], np.int64)
        _, levels, _ = picture(ctx, env.reshape(-1), np.array([0, n], np.int64), C8, span, W, pp.POOLS[pool], _lib.MEM_HOST)
        assert image.shape == (height, W) and image.dtype == np.uint8
        assert np.array_equal(image, np.repeat(levels[0], ratios, axis=0))


# ---- the command ----
def test_plot_gtg_writes_the_picture_of_a_direct_call(ctx, tmp_path, monkeypatch):
    from scipy.io import wavfile
    monkeypatch.chdir(tmp_path)
    n, W = 8000, 300
    wave = speechlike.make(77, n, family="syllables")[0]
    wav = str(tmp_path / "DR1.FXYZ0.SA1.WAV")
    wavfile.write(wav, 16000, wave)
    assert cli.main(["plot", "gtg", "--file", wav, "--width", str(W)]) == 0
    out = os.path.join("graphs", "gtg", "DR1.FXYZ0.SA1.png")
    got = decode_png(open(out, "rb").read())
    assert got.shape == (941, W, 3)

    from f2cnn_amd.scripts.processing.GammatoneFiltering import filterbank_from_config
    cf, coefs = filterbank_from_config()
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    levels = np.zeros((1, 128, W), np.uint8)
    ctx.gammatonegram_batch(wave, _lib.WAVE_I16, np.array([0, n], np.int64), coefs, 1, 128, False, 0.0, _lib.FFT_F32, None, W, 0, None,
                            levels, _lib.MEM_HOST)
    _, ratios = pp.GetNewHeightERB(levels[0], cf)
    plain = pp.colour_table()[np.repeat(levels[0], ratios, axis=0)]
    assert np.array_equal(got, plain) and levels.min() >= 1 and levels.max() == 255

    # with a hand-written .FB (50 frames of 10 ms: F1..F4 flat, F2 with a step) next to it, black pixels in the frames' columns
    frames = np.tile(np.array([0.5, 1.5, 2.5, 3.5, 0.1, 0.1, 0.1, 0.1], np.float32), (50, 1))
    frames[25:, 1] = 1.9
    with open(str(tmp_path / "DR1.FXYZ0.SA1.FB"), "wb") as f:
        f.write(struct.pack('>iihh', 50, 100000, 32, 9) + frames.astype('>f4').tobytes())
    out2 = str(tmp_path / "with_formants.png")
    assert cli.main(["plot", "gtg", "--file", wav, "--width", str(W), "--out", out2]) == 0
    marked = decode_png(open(out2, "rb").read())
    black = (marked == 0).all(axis=2)
    assert np.flatnonzero(black.any(axis=0)).tolist() == [6 * j for j in range(50)]       # frame j: sample 160 j -> column 6 j
    assert np.array_equal(marked[~black], plain[~black])
    rows = sorted(pp.formant_row(f, 941) for f in (500.0, 1500.0, 2500.0, 3500.0))
    assert np.flatnonzero(black[:, 6]).tolist() == rows
    step = np.flatnonzero(black[:, 150])                                               # F2's step at frame 25: a vertical run
    assert set(range(pp.formant_row(1900.0, 941), pp.formant_row(1500.0, 941) + 1)) <= set(step.tolist())
    # one track only, a span in samples, maximum pooling
    out3 = str(tmp_path / "f2.png")
    assert cli.main(["plot", "gtg", "--file", wav, "--width", "100", "--pool", "max", "--formant", "2", "--start", "1600", "--end", "6400",
                     "--out", out3]) == 0
    f2 = decode_png(open(out3, "rb").read())
    assert f2.shape == (941, 100, 3)
    black = (f2 == 0).all(axis=2)
    assert np.flatnonzero(black.any(axis=0)).tolist() == sorted({(160 * j - 1600) * 100 // 4800 for j in range(10, 40)})
    # a file that cannot be read: reported, skipped, exit status 2
    assert cli.main(["plot", "gtg", "--file", str(tmp_path / "absent.WAV")]) == 2
