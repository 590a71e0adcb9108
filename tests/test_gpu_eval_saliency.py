"""f2_eval_saliency_batch. The fused call is defined by calls that exist - f2_eval_figure_batch (scores, labels, window offsets,
levels, range), f2_input_batch + f2_cnn_input_gradient + f2_saliency_map (map, summary) - so every comparison is on raw bits. Then
an utterance too short for a window, the optional outputs, argument errors, and saliency=None through EvaluateWavArrays."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

C, RADIUS, STEP, R = 128, 5, 160, 11
LENGTHS = (4000, 2500)
HOPS = (160, 16)
MEMS = (_lib.MEM_HOST, _lib.MEM_DEVICE)
WIDTH = 50
SEED = 5


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
    waves = [orc.synth_utterance(seed + i, n) for i, n in enumerate(lengths)]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    flat = np.concatenate(waves).astype(np.int16) if sum(lengths) else np.zeros(0, np.int16)
    return flat, offsets


def fill(shape, dtype, byte):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = byte
    return a


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def counts(lengths, hop):
    return [_lib.strided_window_count(int(n), RADIUS, STEP, hop) for n in lengths]


def saliency(ctx, model, coefs, flat, offsets, hop, spans, W, mem):
    """f2_eval_saliency_batch in `mem`, every output pre-filled -> dict(sc, lb, wo, lv, rg, mp, sm)"""
    B = len(offsets) - 1
    total = sum(counts(np.diff(offsets), hop))
    o = dict(sc=fill((total, 2), np.float32, 0x5A), lb=fill((total,), np.uint8, 0x5A), lv=fill((B, C, W), np.uint8, 0xA5),
             mp=fill((B, C, W, 3), np.float64, 0x5A), sm=fill((B, C, 3), np.float64, 0x5A), rg=fill((B, 2), np.float64, 0x5A))
    args = (coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, spans, W, 0)
    h = model.handle(ctx)
    if mem == _lib.MEM_HOST:
        o["wo"], _ = ctx.eval_saliency_batch(h, flat, _lib.WAVE_I16, offsets, *args, o["lv"], o["mp"], o["sm"], o["sc"], o["lb"], mem,
                                             range_out=o["rg"])
    else:
        host = (flat, o["lv"], o["mp"], o["sm"], o["sc"], o["lb"])
        dev = [ctx.malloc(max(a.nbytes, 8)) for a in host]
        try:
            for d, a in zip(dev, host):
                ctx.h2d(d, a)
            o["wo"], _ = ctx.eval_saliency_batch(h, dev[0], _lib.WAVE_I16, offsets, *args, *dev[1:], mem, range_out=o["rg"])
            for d, a in zip(dev[1:], host[1:]):
                if a.size:
                    ctx.d2h(a, d)
        finally:
            ctx.synchronize()
            for d in dev:
                ctx.free(d)
    assert o["wo"][-1] == total
    return o


_parts = {}


def defining_calls(ctx, model, coefs, flat, offsets, hop):
    """the calls that define the fused one, each made once per (batch, hop), all in host memory"""
    key = (flat.size, hop)
    if key in _parts:
        return _parts[key]
    B, lengths, h = len(offsets) - 1, np.diff(offsets), model.handle(ctx)
    nbh = counts(lengths, hop)
    total = sum(nbh)
    spans = np.array([[0, n] for n in lengths], np.int64)
    sc, lb, lv = np.empty((total, 2), np.float32), np.empty(total, np.uint8), np.empty((B, C, WIDTH), np.uint8)
    wo, rg = ctx.eval_figure_batch(h, flat, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, spans, WIDTH, 0,
                                   lv, None, sc, lb, _lib.MEM_HOST)
    centres = np.concatenate([RADIUS * STEP + hop * np.arange(n, dtype=np.int64) for n in nbh] + [np.zeros(0, np.int64)])
    windows = np.empty((total, R, C), np.float32)
    if total:
        ctx.input_batch(flat, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, wo, centres, RADIUS, STEP, True, windows, _lib.MEM_HOST)
    profile = np.empty((total, C, 2))
    ctx.cnn_input_gradient(h, windows, total, None, profile, None, _lib.MEM_HOST)
    mp = ctx.saliency_map(profile, wo, C, spans, RADIUS * STEP, hop, WIDTH, np.empty((B, C, WIDTH, 3)), _lib.MEM_HOST)
    sm = ctx.saliency_map(profile, wo, C, spans, RADIUS * STEP, hop, 1, np.empty((B, C, 1, 3)), _lib.MEM_HOST).reshape(B, C, 3)
    _parts[key] = dict(figure=(sc, lb, wo, lv, rg.copy()), spans=spans, profile=profile, mp=mp, sm=sm)
    return _parts[key]


@pytest.mark.parametrize("hop", HOPS)
def test_fused_call_is_its_defining_calls(ctx, model, coefs, hop):
    flat, offsets = batch_of(LENGTHS)
    want = defining_calls(ctx, model, coefs, flat, offsets, hop)
    sc, lb, wo, lv, rg = want["figure"]
    assert wo[-1] > 0 and np.abs(want["profile"][..., 0]).max() > 0
    for mem in MEMS:
        o = saliency(ctx, model, coefs, flat, offsets, hop, want["spans"], WIDTH, mem)
        assert np.array_equal(o["wo"], wo)
        assert np.array_equal(bits(o["sc"]), bits(sc)) and np.array_equal(o["lb"], lb)
        assert np.array_equal(o["lv"], lv) and np.array_equal(bits(o["rg"]), bits(rg))
        assert np.array_equal(bits(o["mp"]), bits(want["mp"])) and np.array_equal(bits(o["sm"]), bits(want["sm"]))
        assert (o["sm"][:, :, 0] == np.diff(wo)[:, None]).all() and (o["mp"][..., 0].sum(axis=2) == np.diff(wo)[:, None]).all()
        assert (o["sm"][..., 2] >= np.abs(o["sm"][..., 1])).all()                # |sum G x| <= sum |G|: a normalised x lies in [0, 1]


def test_an_utterance_too_short_for_a_window_gets_its_picture_and_an_empty_map(ctx, model, coefs):
    lengths = (4000, 1700, 0)
    flat, offsets = batch_of(lengths)
    for mem in MEMS:
        o = saliency(ctx, model, coefs, flat, offsets, 160, None, 7, mem)
        assert np.diff(o["wo"]).tolist() == counts(lengths, 160) and np.diff(o["wo"])[1] == 0
        assert o["lv"][1].any() and not o["lv"][2].any()
        for u in (1, 2):
            assert (o["mp"][u, :, :, 0] == 0).all() and np.isnan(o["mp"][u, :, :, 1:]).all()
            assert (o["sm"][u, :, 0] == 0).all() and np.isnan(o["sm"][u, :, 1:]).all()
        assert (o["sm"][0, :, 0] == o["wo"][1]).all() and not np.isnan(o["sm"][0]).any()


def test_optional_outputs(ctx, model, coefs):
    flat, offsets = batch_of(LENGTHS)
    want = defining_calls(ctx, model, coefs, flat, offsets, 160)
    B, h = len(LENGTHS), model.handle(ctx)
    args = (coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, 160, want["spans"], WIDTH, 0)
    sm = fill((B, C, 3), np.float64, 0x5A)
    wo, _ = ctx.eval_saliency_batch(h, flat, _lib.WAVE_I16, offsets, *args, None, None, sm, None, None, _lib.MEM_HOST)       # the summary alone
    assert np.array_equal(wo, want["figure"][2]) and np.array_equal(bits(sm), bits(want["sm"]))
    sc = fill((int(wo[-1]), 2), np.float32, 0x5A)
    ctx.eval_saliency_batch(h, flat, _lib.WAVE_I16, offsets, *args, None, None, None, sc, None, _lib.MEM_HOST)               # no map at all
    assert np.array_equal(bits(sc), bits(want["figure"][0]))
    mp = fill((B, C, WIDTH, 3), np.float64, 0x5A)
    ctx.eval_saliency_batch(h, flat, _lib.WAVE_I16, offsets, *args, None, mp, None, None, None, _lib.MEM_HOST)               # the map alone
    assert np.array_equal(bits(mp), bits(want["mp"]))
    for key in ("mp", "sm"):                     # and each of them alone in device memory
        a = fill(want[key].shape, np.float64, 0x5A)
        dw, da = ctx.malloc(flat.nbytes), ctx.malloc(a.nbytes)
        try:
            ctx.h2d(dw, flat)
            ctx.h2d(da, a)
            ctx.eval_saliency_batch(h, dw, _lib.WAVE_I16, offsets, *args, None, da if key == "mp" else None, da if key == "sm" else None,
                                    None, None, _lib.MEM_DEVICE)
            ctx.synchronize()
            ctx.d2h(a, da)
        finally:
            ctx.synchronize()
            ctx.free(dw)
            ctx.free(da)
        assert np.array_equal(bits(a), bits(want[key])), key
    lengths = (1700, 0, 900)                     # samples but no window: pictures, a map and a summary over no rows, no scores
    flat2, off2 = batch_of(lengths)
    for mem in MEMS:
        o = saliency(ctx, model, coefs, flat2, off2, 160, None, 7, mem)
        assert not o["wo"].any() and (o["mp"][..., 0] == 0).all() and np.isnan(o["mp"][..., 1:]).all()
        assert (o["sm"][..., 0] == 0).all() and np.isnan(o["sm"][..., 1:]).all()
        assert [o["lv"][b].any() for b in range(len(lengths))] == [n > 0 for n in lengths]
    wo, rg = ctx.eval_saliency_batch(h, None, _lib.WAVE_I16, np.zeros(1, np.int64), coefs, 0, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, 5,
                                     None, 7, 0, None, None, None, None, None, _lib.MEM_HOST)
    assert wo.tolist() == [0] and rg.shape == (0, 2)


def test_argument_errors_write_nothing(ctx, model, coefs):
    flat, offsets = batch_of(LENGTHS)
    B, W, hop0 = len(LENGTHS), 7, 160
    total = sum(counts(LENGTHS, hop0))
    outs = dict(lv=fill((B, C, W), np.uint8, 0xA5), rg=fill((B, 2), np.float64, 0x5A), mp=fill((B, C, W, 3), np.float64, 0x5A),
                sm=fill((B, C, 3), np.float64, 0x5A), sc=fill((total, 2), np.float32, 0x5A), lb=fill((total,), np.uint8, 0x5A),
                wo=fill(B + 1, np.int64, 0x5A))
    before = {k: v.copy() for k, v in outs.items()}
    A = lambda a: None if a is None else a.ctypes.data

    def call(c=ctx.handle, cnn=model.handle(ctx), wave=flat, dt=_lib.WAVE_I16, off=offsets, co=coefs, B=B, Cn=C, lpf=0, cut=0.0,
             fft=_lib.FFT_F32, radius=RADIUS, step=STEP, hop=hop0, spans=None, W=W, pool=0, mem=_lib.MEM_HOST):
        return ctx.lib.f2_eval_saliency_batch(c, cnn, A(wave), dt, A(off), A(co), B, Cn, lpf, cut, fft, radius, step, hop, A(spans), W, pool,
                                              A(outs["lv"]), A(outs["rg"]), A(outs["mp"]), A(outs["sm"]), A(outs["sc"]), A(outs["lb"]),
                                              A(outs["wo"]), mem)

    down = offsets.copy()
    down[2] = down[1] - 1
    whole = np.array([[0, n] for n in LENGTHS], np.int64)
    past, back, neg = whole.copy(), whole.copy(), whole.copy()
    past[0, 1] += 1
    back[1] = (10, 9)
    neg[1, 0] = -1
    for kw in [dict(c=None), dict(cnn=None), dict(wave=None), dict(dt=7), dict(off=None), dict(off=offsets + 1), dict(off=down),
               dict(co=None), dict(B=-1), dict(Cn=0), dict(Cn=64), dict(lpf=1, cut=0.0), dict(lpf=1, cut=8000.0), dict(fft=5),
               dict(radius=-1), dict(radius=4), dict(step=-1), dict(hop=0), dict(mem=3), dict(mem=_lib.MEM_HOST_ASYNC),
               dict(W=0), dict(pool=2), dict(pool=-1), dict(spans=past), dict(spans=back), dict(spans=neg)]:
        assert call(**kw) == _lib.F2_ERR_INVALID, kw
    assert call(W=65537) == _lib.F2_ERR_UNSUPPORTED
    for k in outs:
        assert np.array_equal(bits(outs[k]), bits(before[k])), k
    assert call() == _lib.F2_OK and outs["wo"][-1] == total and not np.array_equal(bits(outs["sm"]), bits(before["sm"]))


def test_saliency_none_returns_todays_tuples(ctx, model):
    from f2cnn_amd.scripts.CNN import Evaluating
    waves = [orc.synth_utterance(60 + i, n) for i, n in enumerate(LENGTHS)]
    plain = Evaluating.EvaluateWavArrays(waves, 16000, model=model, ctx=ctx, hop=160)
    none = Evaluating.EvaluateWavArrays(waves, 16000, model=model, ctx=ctx, hop=160, saliency=None)
    with_map = Evaluating.EvaluateWavArrays(waves, 16000, model=model, ctx=ctx, hop=160, saliency=True, saliency_width=WIDTH)
    assert len(plain) == len(none) == len(with_map) == len(LENGTHS)
    for p, q, s in zip(plain, none, with_map):
        assert len(p) == len(q) == 2 and len(s) == 3
        for a, b, c in zip(p, q, s):
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
        assert s[2]["summary"].shape == (C, 3) and s[2]["map"].shape == (C, WIDTH, 3) and s[2]["levels"].shape == (C, WIDTH)


# ---- the command --------------------------------------------------------------------------------------------------------------
FIG_W = 200
UPPER = 941                                      # image rows of 128 ERB channels (tests/test_gtg_host.py)
SAL_KEYS = ["saliency_map", "saliency_span", "saliency_summary"]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """resources/f2cnn/TEST/ under a fresh root: one 1.2 s file with .FB / .PHN, one short file without, the configuration"""
    import os
    import label_referee as lr
    from f2cnn_amd import config, wavio
    root = tmp_path_factory.mktemp("salcorpus")
    config.write_default(str(root / "configF2CNN.conf"))
    folder = root / "resources" / "f2cnn" / "TEST"
    os.makedirs(folder)
    wav = lr.write_labelled_file(folder, lambda n: orc.synth_utterance(21, n))
    bare = str(folder / "DR1.NOFB0.SA2.WAV")
    wavio.write_sphere(bare, 16000, orc.synth_utterance(3, 4000))
    return root, wav, bare, F2CNNModel(orc.glorot_weights(SEED))


def read_png(path):
    from test_gtg_host import decode_png
    with open(path, "rb") as f:
        return decode_png(f.read())


def test_eval_saliency_command(corpus, monkeypatch, capsys):
    import os
    from f2cnn_amd import cli
    from f2cnn_amd.scripts.CNN import Evaluating
    root, wav, _, model = corpus
    monkeypatch.chdir(root)
    model.save("last_trained_model")
    npz_path = os.path.splitext(wav)[0] + ".F2CNN.npz"
    sc0, lb0 = Evaluating.EvaluateOneWavFile(wav, hop=160, model=model)
    plain = dict(np.load(npz_path))
    capsys.readouterr()
    assert cli.main(["cnn", "eval", "--file", wav, "--hop", "frame", "--saliency", "--figure-width", str(FIG_W)]) == 0
    printed = capsys.readouterr().out
    got = dict(np.load(npz_path))
    assert sorted(got) == sorted(list(plain) + SAL_KEYS)
    for key in plain:
        assert np.array_equal(bits(got[key]), bits(plain[key])), key
    assert got["saliency_map"].shape == (C, FIG_W, 3) and got["saliency_summary"].shape == (C, 3)
    assert got["saliency_span"].tolist() == [0, 19200]
    assert (got["saliency_summary"][:, 0] == len(lb0)).all() and (got["saliency_map"][:, :, 0].sum(axis=1) == len(lb0)).all()
    assert np.abs(got["saliency_summary"][:, 1]).max() > 0 and (got["saliency_summary"][:, 2] > 0).all()
    rgb = read_png(os.path.join("graphs", "Saliency", "DR1.FSYN0.SA1.png"))
    assert rgb.shape == (2 * UPPER + 8, FIG_W, 3)
    lines = [line for line in printed.splitlines() if line.startswith("\t\t")]
    assert "saliency map -> " in printed and "sum G x" in printed and "sum |G|" in printed
    table = [line.split() for line in lines if len(line.split()) == 5 and "-" in line.split()[1]]
    assert len(table) == C // 8                                               # one line per 8 channels
    assert np.isclose(sum(float(t[3]) for t in table), got["saliency_summary"][:, 1].sum(), atol=1e-6 * len(table))


def test_evalnoise_and_evalrand_saliency(corpus, monkeypatch, capsys):
    import os
    from f2cnn_amd.scripts.CNN import Evaluating
    root, wav, bare, model = corpus
    monkeypatch.chdir(root)
    Evaluating.EvaluateWithNoise(wav, SNRdB=10, model=model, hop=160, rng=np.random.default_rng(5), saliency=16, figure=True, figure_width=64)
    assert read_png(os.path.join("graphs", "Saliency", "DR1.FSYN0.SA110dB.png")).shape == (2 * UPPER + 8, 64, 3)
    noisy = np.load(os.path.join("OutputWavFiles", "addedNoise", "DR1.FSYN0.SA110dB.F2CNN.npz"))
    assert "figure_track" in noisy and noisy["saliency_map"].shape == (C, 64, 3)
    singles = {}
    for file in (wav, bare):
        Evaluating.EvaluateOneWavFile(file, hop=160, model=model, saliency=True, figure_width=64)
        singles[file] = dict(np.load(os.path.splitext(file)[0] + ".F2CNN.npz"))
    capsys.readouterr()
    results = Evaluating.EvaluateRandom(model=model, hop=160, saliency=True, figure_width=64)            # both files: one batched call
    printed = capsys.readouterr().out
    assert sorted(os.path.abspath(str(f)) for f in results) == sorted([wav, bare])
    for file in (wav, bare):
        got = dict(np.load(os.path.splitext(file)[0] + ".F2CNN.npz"))
        assert sorted(got) == sorted(singles[file])
        for key in got:
            assert np.array_equal(bits(got[key]), bits(singles[file][key])), (file, key)
    assert "all files\tsaliency" in printed
    both = Evaluating.CombineSaliencySummaries([singles[f]["saliency_summary"] for f in (wav, bare)])
    assert both[0, 0] == sum(len(results[f][1]) for f in results)
