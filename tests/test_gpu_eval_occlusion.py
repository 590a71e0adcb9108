"""f2_eval_occlusion_batch and `cnn eval|evalnoise|evalrand --occlusion`. The fused call is defined by calls that exist -
f2_eval_batch_strided (level 0), f2_input_batch + f2_occlude_windows' definition in NumPy + f2_cnn_forward (the other levels),
f2_eval_figure_batch (levels, range), f2_occlusion_map (map, summary) - so every comparison is on raw bits; the oracle CNN on the
CPU holds all levels to 2e-5. Then known answers, argument errors, and the command: PNG, table, .npz keys, scores and labels
unchanged by the flag."""
import os

import numpy as np
import pytest

import f2cnn_oracle as orc
import label_referee as lr
import speechlike
from f2cnn_amd import _lib, wavio
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.scripts.CNN.Evaluating import OcclusionPatches
from test_gtg_host import decode_png

pytestmark = pytest.mark.gpu

C, RADIUS, STEP, R = 128, 5, 160, 11
LENGTHS = (1761, 4000, 1700, 0, 6000)          # one window, speech-shaped, no window, empty, the longest (tests/test_gpu_eval_figure.py)
HOPS = (5, 160)
MEMS = (_lib.MEM_HOST, _lib.MEM_DEVICE)
UPPER = 941                                      # image rows of 128 ERB channels (tests/test_gtg_host.py)
SEED = 5                                         # of the weights: see test_the_oracle_sees_flips_and_non_flips
ATOL = 2e-5                                      # of test_cnn_forward_vs_oracle
# 16 bands of 8 channels; 2 row bands x 15 channel bands, the full window and one cell: 32 patches, L = 33 - at hop 5 the batch's
# 1297 windows are three CNN chunks of 16384 // 33 = 496, at hop 1 the longest utterance's 4240 x 33 level-windows pass 131072
PATCHES = {"bands": OcclusionPatches(R, C, 8, 8),
           "grid": np.concatenate([OcclusionPatches(R, C, 16, 8, 6, 5), np.array([[0, R, 0, C], [0, 1, 0, 1]], np.int32)])}
FULL = 30                                        # the full-window patch of "grid"
FILL = {"bands": 0.0, "grid": 0.25}
SPAN, WIDTH = (900, 1500), 50


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))


@pytest.fixture(scope="module")
def model():
    return F2CNNModel(orc.glorot_weights(SEED))


def batch_of(lengths, seed=60):
    waves = [speechlike.make(seed + i, n, "syllables")[0] if n == 4000 else orc.synth_utterance(seed + i, n)
             for i, n in enumerate(lengths)]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.concatenate(waves).astype(np.int16), offsets


def spans_of(lengths):
    return np.array([list(SPAN) if n >= SPAN[1] else [0, n] for n in lengths], np.int64)


def fill(shape, dtype, byte):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = byte
    return a


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def counts(lengths, hop):
    return [_lib.strided_window_count(int(n), RADIUS, STEP, hop) for n in lengths]


def occlusion(ctx, model, coefs, flat, offsets, hop, patches, fillv, spans, W, mem):
    """f2_eval_occlusion_batch in `mem`, every output pre-filled -> dict(sc, lb, wo, lv, rg, mp, sm)"""
    B, K = len(offsets) - 1, len(patches)
    total = sum(counts(np.diff(offsets), hop))
    o = dict(sc=fill((total, K + 1, 2), np.float32, 0x5A), lb=fill((total, K + 1), np.uint8, 0x5A), lv=fill((B, C, W), np.uint8, 0xA5),
             mp=fill((B, K, W, 4), np.float64, 0x5A), sm=fill((B, K, 4), np.float64, 0x5A), rg=fill((B, 2), np.float64, 0x5A))
    args = (coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, patches, fillv, spans, W, 0)
    h = model.handle(ctx)
    if mem == _lib.MEM_HOST:
        o["wo"], _ = ctx.eval_occlusion_batch(h, flat, _lib.WAVE_I16, offsets, *args, o["lv"], o["mp"], o["sm"], o["sc"], o["lb"], mem,
                                              range_out=o["rg"])
    else:
        host = (flat, o["lv"], o["mp"], o["sm"], o["sc"], o["lb"])
        dev = [ctx.malloc(max(a.nbytes, 8)) for a in host]
        try:
            for d, a in zip(dev, host):
                ctx.h2d(d, a)
            o["wo"], _ = ctx.eval_occlusion_batch(h, dev[0], _lib.WAVE_I16, offsets, *args, *dev[1:], mem, range_out=o["rg"])
            for d, a in zip(dev[1:], host[1:]):
                if a.size:
                    ctx.d2h(a, d)
        finally:
            ctx.synchronize()
            for d in dev:
                ctx.free(d)
    assert o["wo"][-1] == total
    return o


def numpy_occlude(x, patches, fillv):
    out = np.repeat(x[:, None], len(patches) + 1, axis=1)
    for k, (r0, r1, c0, c1) in enumerate(patches):
        out[:, k + 1, r0:r1, c0:c1] = np.float32(fillv)
    return out


_parts = {}


def defining_calls(ctx, model, coefs, flat, offsets, hop, name):
    """the calls that define the fused one, each made once per (batch, hop, patch set), all in host memory:
    strided (sc, lb, wo); windows of f2_input_batch; forward = f2_cnn_forward of the NumPy-occluded windows; figure (lv, rg);
    map and summary = f2_occlusion_map of forward's scores and labels"""
    key = (flat.size, hop, name)
    if key in _parts:
        return _parts[key]
    B, lengths, h = len(offsets) - 1, np.diff(offsets), model.handle(ctx)
    patches, fillv = PATCHES[name], FILL[name]
    nbh = counts(lengths, hop)
    total, K = sum(nbh), len(patches)
    sc, lb = np.empty((total, 2), np.float32), np.empty(total, np.uint8)
    wo = ctx.eval_batch_strided(h, flat, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, sc, lb, _lib.MEM_HOST)
    centres = np.concatenate([RADIUS * STEP + hop * np.arange(n, dtype=np.int64) for n in nbh])
    windows = np.empty((total, R, C), np.float32)
    ctx.input_batch(flat, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, wo, centres, RADIUS, STEP, True, windows, _lib.MEM_HOST)
    occluded = numpy_occlude(windows, patches, fillv)
    fsc, flb = np.empty((total, K + 1, 2), np.float32), np.empty((total, K + 1), np.uint8)
    ctx.cnn_forward(h, occluded.reshape(-1, R, C), total * (K + 1), fsc, flb, _lib.MEM_HOST)
    spans, whole = spans_of(lengths), np.array([[0, n] for n in lengths], np.int64)
    lv = np.empty((B, C, WIDTH), np.uint8)
    _, rg = ctx.eval_figure_batch(h, flat, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, spans, WIDTH, 0,
                                  lv, None, None, None, _lib.MEM_HOST)
    _parts[key] = dict(strided=(sc, lb, wo), windows=windows, occluded=occluded, forward=(fsc, flb), figure=(lv, rg.copy()), spans=spans,
                       whole=whole, exact=np.array_equal(bits(fsc[:, 0]), bits(sc)))
    return _parts[key]


def check_against(o, want, patches, hop, ctx):
    """checks 1, 2, 4, 5 of the issue for one result of the fused call"""
    sc, lb, wo = want["strided"]
    fsc, flb = want["forward"]
    K = len(patches)
    assert np.array_equal(o["wo"], wo)
    assert np.array_equal(bits(o["sc"][:, 0]), bits(sc)) and np.array_equal(o["lb"][:, 0], lb)                   # 1
    if want["exact"]:                                                                                            # 2
        assert np.array_equal(bits(o["sc"]), bits(fsc)) and np.array_equal(o["lb"], flb)
    else:
        print("f2_cnn_forward of the f2_input_batch windows is not the strided call's scores bit for bit: levels >= 1 held to", ATOL)
        assert np.allclose(o["sc"], fsc, rtol=0, atol=ATOL)
    assert np.array_equal(o["lb"] != 0, o["sc"][..., 1] > o["sc"][..., 0])                                       # 4
    lv, rg = want["figure"]                                                                                      # 5
    assert np.array_equal(o["lv"], lv) and np.array_equal(bits(o["rg"]), bits(rg))
    B = len(wo) - 1
    mp = ctx.occlusion_map(o["sc"], o["lb"], wo, K, want["spans"], RADIUS * STEP, hop, WIDTH, np.empty((B, K, WIDTH, 4)), _lib.MEM_HOST)
    sm = ctx.occlusion_map(o["sc"], o["lb"], wo, K, want["whole"], RADIUS * STEP, hop, 1, np.empty((B, K, 1, 4)), _lib.MEM_HOST)
    assert np.array_equal(bits(o["mp"]), bits(mp)) and np.array_equal(bits(o["sm"]), bits(sm.reshape(B, K, 4)))
    assert o["sm"][:, :, 0].sum() == K * wo[-1] and (o["sm"][2, :, 0] == 0).all() and np.isnan(o["sm"][2, :, 2:]).all()


def oracle_scores(want, step=1):
    """orc.cnn_forward of every level of every step-th window"""
    x = want["occluded"][::step]
    return orc.cnn_forward(x.reshape(-1, R, C), orc.glorot_weights(SEED)).reshape(x.shape[0], x.shape[1], 2)


def test_the_oracle_sees_flips_and_non_flips(ctx, model, coefs):
    """the condition the issue sets for the seed, on the oracle's scores alone: at least one (window, patch) flips the label
    with both margins above 4e-5, at least one keeps it with both margins above 4e-5 (so that the device's 2e-5 agrees)"""
    flat, offsets = batch_of(LENGTHS)
    s = oracle_scores(defining_calls(ctx, model, coefs, flat, offsets, 160, "bands"))
    m = s[..., 1] - s[..., 0]
    strong = (np.abs(m[:, 1:]) > 4e-5) & (np.abs(m[:, :1]) > 4e-5)
    flip = (m[:, 1:] > 0) != (m[:, :1] > 0)
    print("strong flips", int((flip & strong).sum()), "strong non-flips", int((~flip & strong).sum()))
    assert (flip & strong).any() and (~flip & strong).any()


@pytest.mark.parametrize("name", sorted(PATCHES))
@pytest.mark.parametrize("hop", HOPS)
def test_fused_call_is_its_defining_calls(ctx, model, coefs, hop, name):
    flat, offsets = batch_of(LENGTHS)
    want = defining_calls(ctx, model, coefs, flat, offsets, hop, name)
    assert want["windows"].min() >= 0.0 and want["windows"].max() <= 1.0
    for mem in MEMS:
        o = occlusion(ctx, model, coefs, flat, offsets, hop, PATCHES[name], FILL[name], want["spans"], WIDTH, mem)
        check_against(o, want, PATCHES[name], hop, ctx)
    step = 1 if hop == 160 else 37                                                                                # 3
    ref = oracle_scores(want, step)
    err = np.abs(o["sc"][::step] - ref).max()
    print(f"hop {hop} {name}: max |score - oracle| {err:.3g} over {ref.shape[0]} windows x {ref.shape[1]} levels")
    assert err <= ATOL
    if hop == 160 and name == "bands":          # the flips the oracle is sure of are the device's
        m = ref[..., 1] - ref[..., 0]
        sure = (np.abs(m[:, 1:]) > 4e-5) & (np.abs(m[:, :1]) > 4e-5)
        flips = (o["lb"][:, 1:] != 0) != (o["lb"][:, :1] != 0)
        assert np.array_equal(flips[sure], ((m[:, 1:] > 0) != (m[:, :1] > 0))[sure]) and flips[sure].any() and not flips[sure].all()
        assert o["sm"][:, :, 1].sum() == flips.sum()
    if name == "grid":                          # 6: the full-window patch leaves nothing of the window: one score for all
        full = o["sc"][:, FULL + 1]
        assert len(full) > 1 and (bits(full).reshape(len(full), -1) == bits(full[:1]).reshape(1, -1)).all()


def test_every_sample_hop_crosses_a_dense_group(ctx, model, coefs):
    flat, offsets = batch_of((6000,), seed=64)
    want = defining_calls(ctx, model, coefs, flat, offsets, 1, "grid")
    n, L = want["forward"][0].shape[:2]
    assert n * L > 131072
    o = occlusion(ctx, model, coefs, flat, offsets, 1, PATCHES["grid"], FILL["grid"], want["spans"], WIDTH, _lib.MEM_DEVICE)
    sc, lb, wo = want["strided"]
    fsc, flb = want["forward"]
    assert np.array_equal(bits(o["sc"][:, 0]), bits(sc)) and np.array_equal(o["lb"][:, 0], lb)
    if want["exact"]:
        assert np.array_equal(bits(o["sc"]), bits(fsc)) and np.array_equal(o["lb"], flb)
    else:
        assert np.allclose(o["sc"], fsc, rtol=0, atol=ATOL)
    ref = oracle_scores(want, 211)
    assert np.abs(o["sc"][::211] - ref).max() <= ATOL
    mp = ctx.occlusion_map(o["sc"], o["lb"], wo, L - 1, want["spans"], RADIUS * STEP, 1, WIDTH, np.empty((1, L - 1, WIDTH, 4)), _lib.MEM_HOST)
    assert np.array_equal(bits(o["mp"]), bits(mp))


def test_a_fill_that_is_already_there_changes_nothing(ctx, model, coefs):
    """A silent utterance: its windows hold a value <= 0, the window stage makes them zeros and the call ends in
    F2_ERR_NONPOSITIVE with its outputs written, as the strided call does. With fill 0 every level of such a window is the
    window: identical scores, no flip, d = 0."""
    speech = speechlike.make(61, 4000, "syllables")[0]
    flat = np.concatenate([np.zeros(2400, np.int16), np.asarray(speech).astype(np.int16)])
    offsets = np.array([0, 2400, 6400], np.int64)
    patches, hop = PATCHES["bands"], 40
    K, n = len(patches), counts(np.diff(offsets), hop)
    sc, lb = fill((sum(n), K + 1, 2), np.float32, 0x5A), fill((sum(n), K + 1), np.uint8, 0x5A)
    sm = fill((2, K, 4), np.float64, 0x5A)
    with pytest.raises(_lib.F2Error) as e:
        ctx.eval_occlusion_batch(model.handle(ctx), flat, _lib.WAVE_I16, offsets, coefs, 2, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop,
                                 patches, 0.0, None, WIDTH, 0, None, None, sm, sc, lb, _lib.MEM_HOST)
    assert e.value.code == _lib.F2_ERR_NONPOSITIVE
    silent = sc[:n[0]]
    assert n[0] > 1 and (bits(silent).reshape(n[0], K + 1, -1) == bits(silent[:, :1]).reshape(n[0], 1, -1)).all()
    assert (lb[:n[0]] == lb[:n[0], :1]).all()
    assert np.array_equal(sm[0], np.tile([n[0], 0.0, 0.0, 0.0], (K, 1)))
    assert (sm[1, :, 0] == n[1]).all() and (sm[1, :, 3] > 0).all()          # the speech beside it does move


def test_optional_outputs_and_empty_batches(ctx, model, coefs):
    flat, offsets = batch_of(LENGTHS)
    want = defining_calls(ctx, model, coefs, flat, offsets, 160, "bands")
    patches, h, B = PATCHES["bands"], model.handle(ctx), len(LENGTHS)
    K = len(patches)
    args = (coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, 160, patches, 0.0, want["spans"], WIDTH, 0)
    full = occlusion(ctx, model, coefs, flat, offsets, 160, patches, 0.0, want["spans"], WIDTH, _lib.MEM_HOST)
    sm = fill((B, K, 4), np.float64, 0x5A)
    wo, _ = ctx.eval_occlusion_batch(h, flat, _lib.WAVE_I16, offsets, *args, None, None, sm, None, None, _lib.MEM_HOST)     # the summary alone
    assert np.array_equal(wo, full["wo"]) and np.array_equal(bits(sm), bits(full["sm"]))
    mp = fill((B, K, WIDTH, 4), np.float64, 0x5A)
    ctx.eval_occlusion_batch(h, flat, _lib.WAVE_I16, offsets, *args, None, mp, None, None, None, _lib.MEM_HOST)             # the map alone
    assert np.array_equal(bits(mp), bits(full["mp"]))
    for key in ("mp", "sm"):                     # and each of them alone in device memory
        a = fill(full[key].shape, np.float64, 0x5A)
        dw, da = ctx.malloc(flat.nbytes), ctx.malloc(a.nbytes)
        try:
            ctx.h2d(dw, flat)
            ctx.h2d(da, a)
            ctx.eval_occlusion_batch(h, dw, _lib.WAVE_I16, offsets, *args, None, da if key == "mp" else None, da if key == "sm" else None,
                                     None, None, _lib.MEM_DEVICE)
            ctx.synchronize()
            ctx.d2h(a, da)
        finally:
            ctx.synchronize()
            ctx.free(dw)
            ctx.free(da)
        assert np.array_equal(bits(a), bits(full[key])), key
    for lengths in ((1700, 0, 900), (0, 0)):     # no window at all: pictures, empty maps, no scores
        flat2, off2 = batch_of(lengths) if sum(lengths) else (np.zeros(0, np.int16), np.zeros(len(lengths) + 1, np.int64))
        for mem in MEMS:
            o = occlusion(ctx, model, coefs, flat2, off2, 5, patches, 0.0, None, 7, mem)
            assert not o["wo"].any() and (o["mp"][..., :2] == 0).all() and np.isnan(o["mp"][..., 2:]).all()
            assert (o["sm"][..., :2] == 0).all() and np.isnan(o["sm"][..., 2:]).all()
            assert [o["lv"][b].any() for b in range(len(lengths))] == [n > 0 for n in lengths]
    wo, rg = ctx.eval_occlusion_batch(h, None, _lib.WAVE_I16, np.zeros(1, np.int64), coefs, 0, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, 5,
                                      patches, 0.0, None, 7, 0, None, None, None, None, None, _lib.MEM_HOST)
    assert wo.tolist() == [0] and rg.shape == (0, 2)


def test_argument_errors_write_nothing(ctx, model, coefs):
    import ctypes
    flat, offsets = batch_of(LENGTHS)
    B, W, hop0, P0 = len(LENGTHS), 7, 160, PATCHES["bands"]
    K0 = len(P0)
    total = sum(counts(LENGTHS, hop0))
    outs = dict(lv=fill((B, C, W), np.uint8, 0xA5), rg=fill((B, 2), np.float64, 0x5A), mp=fill((B, K0, W, 4), np.float64, 0x5A),
                sm=fill((B, K0, 4), np.float64, 0x5A), sc=fill((total, K0 + 1, 2), np.float32, 0x5A),
                lb=fill((total, K0 + 1), np.uint8, 0x5A), wo=fill(B + 1, np.int64, 0x5A))
    before = {k: v.copy() for k, v in outs.items()}
    A = lambda a: None if a is None else a.ctypes.data

    def call(c=ctx.handle, cnn=model.handle(ctx), wave=flat, dt=_lib.WAVE_I16, off=offsets, co=coefs, B=B, Cn=C, lpf=0, cut=0.0,
             fft=_lib.FFT_F32, radius=RADIUS, step=STEP, hop=hop0, P=P0, K=K0, fv=0.0, spans=None, W=W, pool=0, mem=_lib.MEM_HOST):
        return ctx.lib.f2_eval_occlusion_batch(c, cnn, A(wave), dt, A(off), A(co), B, Cn, lpf, cut, fft, radius, step, hop, A(P), K,
                                               ctypes.c_float(fv), A(spans), W, pool, A(outs["lv"]), A(outs["rg"]), A(outs["mp"]),
                                               A(outs["sm"]), A(outs["sc"]), A(outs["lb"]), A(outs["wo"]), mem)

    def patch(k, col, v):
        Q = P0.copy()
        Q[k, col] = v
        return Q

    down = offsets.copy()
    down[2] = down[1] - 1
    whole = np.array([[0, n] for n in LENGTHS], np.int64)
    past, back, neg = whole.copy(), whole.copy(), whole.copy()
    past[0, 1] += 1
    back[1] = (10, 9)
    neg[4, 0] = -1
    figure_errors = [dict(c=None), dict(cnn=None), dict(wave=None), dict(dt=7), dict(off=None), dict(off=offsets + 1), dict(off=down),
                     dict(co=None), dict(B=-1), dict(Cn=0), dict(Cn=64), dict(lpf=1, cut=0.0), dict(lpf=1, cut=8000.0), dict(fft=5),
                     dict(radius=-1), dict(radius=4), dict(step=-1), dict(hop=0), dict(mem=3), dict(mem=_lib.MEM_HOST_ASYNC),
                     dict(W=0), dict(pool=2), dict(pool=-1), dict(spans=past), dict(spans=back), dict(spans=neg)]
    occlusion_errors = [dict(P=None), dict(K=0), dict(K=-1), dict(fv=1.5), dict(fv=-0.25), dict(fv=float("nan")),
                        dict(P=patch(1, 0, -1)), dict(P=patch(2, 1, R + 1)), dict(P=patch(0, 0, R)), dict(P=patch(3, 2, -1)),
                        dict(P=patch(0, 3, C + 1)), dict(P=patch(5, 3, 0))]
    for kw in figure_errors + occlusion_errors:
        assert call(**kw) == _lib.F2_ERR_INVALID, kw
    assert call(W=65537) == _lib.F2_ERR_UNSUPPORTED
    assert call(P=np.tile(P0[:1], (1025, 1)), K=1025) == _lib.F2_ERR_UNSUPPORTED
    for k in outs:
        assert np.array_equal(bits(outs[k]), bits(before[k])), k
    assert call() == _lib.F2_OK and outs["wo"][-1] == total and not np.array_equal(bits(outs["sm"]), bits(before["sm"]))


# ---- the command --------------------------------------------------------------------------------------------------------------
FIG_W = 200
OCC_KEYS = ["occlusion_fill", "occlusion_hz", "occlusion_map", "occlusion_patches", "occlusion_scores", "occlusion_span",
            "occlusion_summary"]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """resources/f2cnn/TEST/ under a fresh root: one 1.2 s file with .FB / .PHN, one short file without, the configuration"""
    from f2cnn_amd import config
    root = tmp_path_factory.mktemp("occcorpus")
    config.write_default(str(root / "configF2CNN.conf"))
    folder = root / "resources" / "f2cnn" / "TEST"
    os.makedirs(folder)
    wav = lr.write_labelled_file(folder, lambda n: orc.synth_utterance(21, n))
    bare = str(folder / "DR1.NOFB0.SA2.WAV")
    wavio.write_sphere(bare, 16000, orc.synth_utterance(3, 4000))
    return root, wav, bare, F2CNNModel(orc.glorot_weights(SEED))


def read_png(path):
    with open(path, "rb") as f:
        return decode_png(f.read())


@pytest.mark.parametrize("hop", (7, None))
def test_eval_occlusion_command(corpus, monkeypatch, capsys, hop):
    from f2cnn_amd.scripts.CNN import Evaluating
    root, wav, _, model = corpus
    monkeypatch.chdir(root)
    npz_path = os.path.splitext(wav)[0] + ".F2CNN.npz"
    sc0, lb0 = Evaluating.EvaluateOneWavFile(wav, hop=hop, model=model)
    plain = dict(np.load(npz_path))
    capsys.readouterr()
    sc, lb = Evaluating.EvaluateOneWavFile(wav, hop=hop, model=model, occlusion=True, figure_width=FIG_W)
    printed = capsys.readouterr().out
    assert np.array_equal(bits(sc), bits(sc0)) and np.array_equal(lb, lb0)
    got = dict(np.load(npz_path))
    assert sorted(got) == sorted(list(plain) + OCC_KEYS)
    for key in plain:
        assert np.array_equal(bits(got[key]), bits(plain[key])), key
    K = 16
    assert got["occlusion_patches"].shape == (K, 4) and got["occlusion_scores"].shape == (len(lb), K + 1, 2)
    assert np.array_equal(bits(got["occlusion_scores"][:, 0]), bits(sc0))
    assert got["occlusion_summary"].shape == (K, 4) and got["occlusion_map"].shape == (K, FIG_W, 4) and got["occlusion_hz"].shape == (K, 2)
    assert got["occlusion_span"].tolist() == [0, 19200] and got["occlusion_fill"] == 0
    assert (got["occlusion_summary"][:, 0] == len(lb)).all() and (got["occlusion_map"][:, :, 0].sum(axis=1) == len(lb)).all()
    assert np.array_equal(got["occlusion_map"][:, :, 1].sum(axis=1), got["occlusion_summary"][:, 1])
    rgb = read_png(os.path.join("graphs", "Occlusion", "DR1.FSYN0.SA1.png"))
    assert rgb.shape == (2 * UPPER + 8, FIG_W, 3)
    assert "occlusion map -> " in printed and printed.count("\n") >= K + 2 and "mean |d|" in printed


def test_row_bands_give_the_table_without_a_picture(corpus, monkeypatch, capsys):
    from f2cnn_amd.scripts.CNN import Evaluating
    root, _, bare, model = corpus
    monkeypatch.chdir(root)
    Evaluating.EvaluateOneWavFile(bare, hop=40, model=model, occlusion=dict(band=32, stride=32, row_band=6, row_stride=5, fill=0.5),
                                  figure_width=64)
    got = dict(np.load(os.path.splitext(bare)[0] + ".F2CNN.npz"))
    assert got["occlusion_patches"].shape == (8, 4) and got["occlusion_fill"] == np.float32(0.5)
    assert not os.path.exists(os.path.join("graphs", "Occlusion", "DR1.NOFB0.SA2.png"))
    assert "no picture" in capsys.readouterr().out


def test_evalnoise_and_evalrand_occlusion(corpus, monkeypatch, capsys):
    from f2cnn_amd.scripts.CNN import Evaluating
    root, wav, bare, model = corpus
    monkeypatch.chdir(root)
    Evaluating.EvaluateWithNoise(wav, SNRdB=10, model=model, hop=160, rng=np.random.default_rng(5), occlusion=(16, 16), figure=True,
                                 figure_width=64)
    assert read_png(os.path.join("graphs", "Occlusion", "DR1.FSYN0.SA110dB.png")).shape == (2 * UPPER + 8, 64, 3)
    noisy = np.load(os.path.join("OutputWavFiles", "addedNoise", "DR1.FSYN0.SA110dB.F2CNN.npz"))
    assert "figure_track" in noisy and noisy["occlusion_patches"].shape == (8, 4)
    singles = {}
    for file in (wav, bare):
        Evaluating.EvaluateOneWavFile(file, hop=160, model=model, occlusion=True, figure_width=64)
        singles[file] = dict(np.load(os.path.splitext(file)[0] + ".F2CNN.npz"))
    capsys.readouterr()
    results = Evaluating.EvaluateRandom(model=model, hop=160, occlusion=True, figure_width=64)          # both files: one batched call
    printed = capsys.readouterr().out
    assert sorted(os.path.abspath(str(f)) for f in results) == sorted([wav, bare])
    for file in (wav, bare):
        got = dict(np.load(os.path.splitext(file)[0] + ".F2CNN.npz"))
        assert sorted(got) == sorted(singles[file])
        for key in got:
            assert np.array_equal(bits(got[key]), bits(singles[file][key])), (file, key)
    assert "all files\tocclusion" in printed
    both = Evaluating.CombineOcclusionSummaries([singles[f]["occlusion_summary"] for f in (wav, bare)])
    assert both[0, 0] == sum(len(results[f][1]) for f in results)
