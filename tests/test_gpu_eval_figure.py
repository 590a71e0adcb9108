"""f2_eval_figure_batch and `cnn eval|evalnoise|evalrand --figure`. The fused call is defined by three calls that exist -
f2_eval_batch_strided, f2_envelope_picture on the envelopes f2_eval_utterance hands out, f2_score_track - so every comparison is
on raw bits. Then argument errors, and the command: PNG, .npz keys, scores and labels unchanged by the flag."""
import os

import numpy as np
import pytest

import f2cnn_oracle as orc
import label_referee as lr
import speechlike
from f2cnn_amd import _lib, wavio
from f2cnn_amd.model import F2CNNModel
from test_gtg_host import decode_png

pytestmark = pytest.mark.gpu

C, RADIUS, STEP = 128, 5, 160
LENGTHS = (1761, 4000, 1700, 0, 6000)          # one window, speech-shaped, no window, empty, the longest
HOPS = (5, 160)
WIDTHS = (1, 50, 300)
SPANS = {"whole": None, "inner": (900, 1500)}   # of every utterance long enough, else its whole length
MEMS = (_lib.MEM_HOST, _lib.MEM_DEVICE)
UPPER = 941                                      # image rows of 128 ERB channels (tests/test_gtg_host.py)


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
    return F2CNNModel(orc.glorot_weights(7))


def batch_of(lengths, seed=60):
    waves = [speechlike.make(seed + i, n, "syllables")[0] if n == 4000 else orc.synth_utterance(seed + i, n)
             for i, n in enumerate(lengths)]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.concatenate(waves).astype(np.int16), offsets


def spans_of(lengths, kind):
    if SPANS[kind] is None:
        return None
    s, e = SPANS[kind]
    return np.array([[s, e] if n >= e else [0, n] for n in lengths], np.int64)


def fill(shape, dtype, byte):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = byte
    return a


def figure(ctx, model, coefs, flat, offsets, lpf, hop, spans, W, mem):
    """f2_eval_figure_batch in `mem`, every output pre-filled with 0x5A / 0xA5 -> scores, labels, wo, levels, range, track"""
    B = len(offsets) - 1
    total = sum(_lib.strided_window_count(int(n), RADIUS, STEP, hop) for n in np.diff(offsets))
    sc, lb = fill((total, 2), np.float32, 0x5A), fill(total, np.uint8, 0x5A)
    lv, tr, rg = fill((B, C, W), np.uint8, 0xA5), fill((B, W, 5), np.float64, 0x5A), fill((B, 2), np.float64, 0x5A)
    args = (coefs, B, C, lpf, 50.0 if lpf else 0.0, _lib.FFT_F32, RADIUS, STEP, hop, spans, W, 0)
    if mem == _lib.MEM_HOST:
        wo, _ = ctx.eval_figure_batch(model.handle(ctx), flat, _lib.WAVE_I16, offsets, *args, lv, tr, sc, lb, mem, range_out=rg)
    else:
        host = (flat, lv, tr, sc, lb)
        dev = [ctx.malloc(max(a.nbytes, 8)) for a in host]
        try:
            for d, a in zip(dev, host):
                ctx.h2d(d, a)
            wo, _ = ctx.eval_figure_batch(model.handle(ctx), dev[0], _lib.WAVE_I16, offsets, *args, dev[1], dev[2], dev[3], dev[4], mem,
                                          range_out=rg)
            for d, a in zip(dev[1:], host[1:]):
                if a.size:
                    ctx.d2h(a, d)
        finally:
            ctx.synchronize()
            for d in dev:
                ctx.free(d)
    assert wo[-1] == total
    return sc, lb, wo, lv, rg, tr


_parts = {}


def defining_calls(ctx, model, coefs, flat, offsets, lpf, hop, kind, W):
    """the three calls that define the fused one, each computed once: (scores, labels, wo), (levels, range), track"""
    B, lengths = len(offsets) - 1, np.diff(offsets)
    cutoff = 50.0 if lpf else 0.0
    key = (flat.size, lpf, hop)
    if key not in _parts:
        total = sum(_lib.strided_window_count(int(n), RADIUS, STEP, hop) for n in lengths)
        sc, lb = np.empty((total, 2), np.float32), np.empty(total, np.uint8)
        wo = ctx.eval_batch_strided(model.handle(ctx), flat, _lib.WAVE_I16, offsets, coefs, B, C, lpf, cutoff, _lib.FFT_F32, RADIUS, STEP,
                                    hop, sc, lb, _lib.MEM_HOST)
        _parts[key] = (sc, lb, wo)
    sc, lb, wo = _parts[key]
    key = (flat.size, lpf, "env")
    if key not in _parts:           # the envelopes the evaluation uses: f2_eval_utterance's env_or_null, utterance by utterance
        env = np.empty(C * int(offsets[-1]))
        for b, n in enumerate(lengths):
            if n:
                e = np.empty((C, int(n)))
                ctx.eval_utterance(model.handle(ctx), flat[offsets[b]:offsets[b + 1]].copy(), _lib.WAVE_I16, int(n), coefs, C, lpf, cutoff,
                                   _lib.FFT_F32, RADIUS, STEP, e, None, None, _lib.MEM_HOST)
                env[C * offsets[b]:C * offsets[b + 1]] = e.reshape(-1)
        _parts[key] = env
    spans = spans_of(lengths, kind)
    key = (flat.size, lpf, kind, W)
    if key not in _parts:
        lv = np.empty((B, C, W), np.uint8)
        _parts[key] = (lv, ctx.envelope_picture(_parts[(flat.size, lpf, "env")], offsets, B, C, spans, W, 0, None, lv, _lib.MEM_HOST).copy())
    whole = np.array([[0, n] for n in lengths], np.int64)
    track = ctx.score_track(sc, lb, wo, whole if spans is None else spans, RADIUS * STEP, hop, W, np.empty((B, W, 5)), _lib.MEM_HOST)
    return (sc, lb, wo), _parts[key], track


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_is_the_three_calls(got, want):
    sc, lb, wo, lv, rg, tr = got
    (sc0, lb0, wo0), (lv0, rg0), tr0 = want
    assert np.array_equal(wo, wo0)
    assert np.array_equal(bits(sc), bits(sc0)) and np.array_equal(lb, lb0)
    assert np.array_equal(lv, lv0) and np.array_equal(bits(rg), bits(rg0))
    assert np.array_equal(bits(tr), bits(tr0))


@pytest.mark.parametrize("kind", sorted(SPANS))
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("lpf", [False, True], ids=["nolpf", "lpf50"])
def test_fused_call_is_its_three_defining_calls(ctx, model, coefs, lpf, hop, W, kind):
    flat, offsets = batch_of(LENGTHS)
    want = defining_calls(ctx, model, coefs, flat, offsets, lpf, hop, kind, W)
    tr0 = want[2]
    assert (tr0[2, :, 0] == 0).all() and np.isnan(tr0[2, :, 2:]).all()          # too short for a window: all empty columns ...
    assert want[1][0][2].any() and want[1][1][2, 1] > 0                          # ... under a picture all the same
    assert tr0[..., 0].sum() == want[0][2][-1] if kind == "whole" else tr0[..., 0].sum() > 0
    for mem in MEMS:
        assert_is_the_three_calls(figure(ctx, model, coefs, flat, offsets, lpf, hop, spans_of(LENGTHS, kind), W, mem), want)


def test_every_sample_hop(ctx, model, coefs):
    flat, offsets = batch_of((4000,), seed=61)
    want = defining_calls(ctx, model, coefs, flat, offsets, True, 1, "inner", 50)
    sc1, lb1 = np.empty_like(want[0][0]), np.empty_like(want[0][1])
    ctx.eval_batch(model.handle(ctx), flat, _lib.WAVE_I16, offsets, coefs, 1, C, True, 50.0, _lib.FFT_F32, RADIUS, STEP, sc1, lb1,
                   _lib.MEM_HOST)
    assert np.array_equal(bits(sc1), bits(want[0][0])) and np.array_equal(lb1, want[0][1])      # hop 1 is f2_eval_batch
    for mem in MEMS:
        assert_is_the_three_calls(figure(ctx, model, coefs, flat, offsets, True, 1, spans_of((4000,), "inner"), 50, mem), want)


def test_optional_outputs_and_empty_batches(ctx, model, coefs):
    flat, offsets = batch_of(LENGTHS)
    want = defining_calls(ctx, model, coefs, flat, offsets, False, 160, "whole", 50)
    h = model.handle(ctx)
    args = (coefs, len(LENGTHS), C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, 160, None, 50, 0)
    tr = fill((len(LENGTHS), 50, 5), np.float64, 0x5A)
    wo, _ = ctx.eval_figure_batch(h, flat, _lib.WAVE_I16, offsets, *args, None, tr, None, None, _lib.MEM_HOST)       # the track alone
    assert np.array_equal(wo, want[0][2]) and np.array_equal(bits(tr), bits(want[2]))
    lv = fill((len(LENGTHS), C, 50), np.uint8, 0xA5)
    wo, rg = ctx.eval_figure_batch(h, flat, _lib.WAVE_I16, offsets, *args, lv, None, None, None, _lib.MEM_HOST)      # the picture alone
    assert np.array_equal(lv, want[1][0]) and np.array_equal(bits(rg), bits(want[1][1]))
    # no utterance long enough for a window: pictures, empty tracks, no scores; no samples at all: levels 0, range (0, 0)
    for lengths in ((1700, 0, 900), (0, 0)):
        flat2, off2 = batch_of(lengths) if sum(lengths) else (np.zeros(0, np.int16), np.zeros(len(lengths) + 1, np.int64))
        for mem in MEMS:
            sc, lb, wo, lv, rg, tr = figure(ctx, model, coefs, flat2, off2, True, 5, None, 7, mem)
            assert not wo.any() and (tr[..., :2] == 0).all() and np.isnan(tr[..., 2:]).all()
            env_rows = [lv[b].any() for b in range(len(lengths))]
            assert env_rows == [n > 0 for n in lengths] and [(r > 0).all() for r in rg] == env_rows
    wo, rg = ctx.eval_figure_batch(h, None, _lib.WAVE_I16, np.zeros(1, np.int64), coefs, 0, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, 5, None,
                                   7, 0, None, None, None, None, _lib.MEM_HOST)
    assert wo.tolist() == [0] and rg.shape == (0, 2)


def test_argument_errors_write_nothing(ctx, model, coefs):
    flat, offsets = batch_of(LENGTHS)
    B, W, hop = len(LENGTHS), 7, 160
    total = sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in LENGTHS)
    outs = dict(lv=fill((B, C, W), np.uint8, 0xA5), rg=fill((B, 2), np.float64, 0x5A), tr=fill((B, W, 5), np.float64, 0x5A),
                sc=fill((total, 2), np.float32, 0x5A), lb=fill(total, np.uint8, 0x5A), wo=fill(B + 1, np.int64, 0x5A))
    before = {k: v.copy() for k, v in outs.items()}
    P = lambda a: None if a is None else a.ctypes.data

    def call(c=ctx.handle, cnn=model.handle(ctx), wave=flat, dt=_lib.WAVE_I16, off=offsets, co=coefs, B=B, Cn=C, lpf=0, cut=0.0,
             fft=_lib.FFT_F32, radius=RADIUS, step=STEP, hop=hop, spans=None, W=W, pool=0, mem=_lib.MEM_HOST):
        return ctx.lib.f2_eval_figure_batch(c, cnn, P(wave), dt, P(off), P(co), B, Cn, lpf, cut, fft, radius, step, hop, P(spans), W, pool,
                                            P(outs["lv"]), P(outs["rg"]), P(outs["tr"]), P(outs["sc"]), P(outs["lb"]), P(outs["wo"]), mem)

    down = offsets.copy()
    down[2] = down[1] - 1
    whole = np.array([[0, n] for n in LENGTHS], np.int64)
    past, back, neg = whole.copy(), whole.copy(), whole.copy()
    past[0, 1] += 1
    back[1] = (10, 9)
    neg[4, 0] = -1
    strided_errors = [dict(c=None), dict(cnn=None), dict(wave=None), dict(dt=7), dict(off=None), dict(off=offsets + 1), dict(off=down),
                      dict(co=None), dict(B=-1), dict(Cn=0), dict(Cn=64), dict(lpf=1, cut=0.0), dict(lpf=1, cut=8000.0), dict(fft=5),
                      dict(radius=-1), dict(radius=4), dict(step=-1), dict(hop=0), dict(mem=3), dict(mem=_lib.MEM_HOST_ASYNC)]
    picture_errors = [dict(W=0), dict(pool=2), dict(pool=-1), dict(spans=past), dict(spans=back), dict(spans=neg)]
    for kw in strided_errors + picture_errors:
        assert call(**kw) == _lib.F2_ERR_INVALID, kw
    assert call(W=65537) == _lib.F2_ERR_UNSUPPORTED
    for k in outs:
        assert np.array_equal(bits(outs[k]), bits(before[k])), k
    assert call() == _lib.F2_OK and outs["wo"][-1] == total and not np.array_equal(bits(outs["tr"]), bits(before["tr"]))


# ---- the command --------------------------------------------------------------------------------------------------------------
FIG_W = 200
TODAY = {None: ["labels", "scores"], 7: ["hop", "labels", "scores", "timepoints"]}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """resources/f2cnn/TEST/ under a fresh root: one 1.2 s file with .FB / .PHN, one short file without, the configuration"""
    from f2cnn_amd import config
    root = tmp_path_factory.mktemp("evalcorpus")
    config.write_default(str(root / "configF2CNN.conf"))
    folder = root / "resources" / "f2cnn" / "TEST"
    os.makedirs(folder)
    wav = lr.write_labelled_file(folder, lambda n: orc.synth_utterance(21, n))
    bare = str(folder / "DR1.NOFB0.SA2.WAV")
    wavio.write_sphere(bare, 16000, orc.synth_utterance(3, 4000))
    return root, wav, bare, F2CNNModel(orc.glorot_weights(7))


def read_png(path):
    with open(path, "rb") as f:
        return decode_png(f.read())


def blue_columns(rgb):
    from f2cnn_amd.scripts.plotting import PlottingCNN as pc
    lower = rgb[UPPER + pc.GAP_ROWS:UPPER + pc.GAP_ROWS + pc.LOWER_ROWS]
    return (lower == np.array(pc.BLUE, np.uint8)).all(axis=2).any(axis=0)


@pytest.mark.parametrize("hop", (7, None))
def test_eval_figure_command(corpus, monkeypatch, capsys, hop):
    from f2cnn_amd.scripts.CNN import Evaluating
    from f2cnn_amd.scripts.plotting import PlottingCNN as pc
    root, wav, _, model = corpus
    monkeypatch.chdir(root)
    npz_path = os.path.splitext(wav)[0] + ".F2CNN.npz"
    capsys.readouterr()
    sc0, lb0 = Evaluating.EvaluateOneWavFile(wav, hop=hop, model=model)
    plain, printed = dict(np.load(npz_path)), capsys.readouterr().out
    assert sorted(plain) == TODAY[hop] and "figure" not in printed.replace("configF2CNN", "")
    sc, lb = Evaluating.EvaluateOneWavFile(wav, hop=hop, model=model, figure=True, figure_width=FIG_W, accuracy="centre")
    assert np.array_equal(bits(sc), bits(sc0)) and np.array_equal(lb, lb0)
    got = dict(np.load(npz_path))
    assert sorted(got) == sorted(TODAY[hop] + ["accuracy", "accuracy_mode", "confusion", "figure_span", "figure_track"])
    assert np.array_equal(bits(got["scores"]), bits(plain["scores"])) and np.array_equal(got["labels"], plain["labels"])
    track = got["figure_track"]
    assert track.shape == (FIG_W, 5) and got["figure_span"].tolist() == [0, 19200]
    assert track[:, 0].sum() == len(lb) and track[:, 1].sum() == int(lb.sum())
    rgb = read_png(os.path.join("graphs", "FallingOrRising", "DR1.FSYN0.SA1.png"))
    assert rgb.shape == (UPPER + 8 + 321 + 12, FIG_W, 3)
    assert np.array_equal(blue_columns(rgb), track[:, 0] > 0)          # the curve stands in exactly the columns with decisions
    lower = rgb[UPPER + 8:UPPER + 8 + 321]
    assert (lower == np.array(pc.GREEN, np.uint8)).all(axis=2).any()   # the slope of the .FB track
    assert "figure -> " in capsys.readouterr().out


def test_a_file_without_side_files_still_gets_picture_and_curve(corpus, monkeypatch, capsys):
    from f2cnn_amd.scripts.CNN import Evaluating
    from f2cnn_amd.scripts.plotting import PlottingCNN as pc
    root, _, bare, model = corpus
    monkeypatch.chdir(root)
    _, lb = Evaluating.EvaluateOneWavFile(bare, hop=7, model=model, figure=True, figure_width=64)
    got = dict(np.load(os.path.splitext(bare)[0] + ".F2CNN.npz"))
    assert sorted(got) == sorted(TODAY[7] + ["figure_span", "figure_track"]) and got["figure_track"][:, 0].sum() == len(lb) > 0
    rgb = read_png(os.path.join("graphs", "FallingOrRising", "DR1.NOFB0.SA2.png"))
    assert rgb.shape == (UPPER + 8 + 321 + 12, 64, 3) and blue_columns(rgb).any()
    assert len(np.unique(rgb[:UPPER].reshape(-1, 3), axis=0)) > 16     # a gammatonegram, not a blank
    lower = rgb[UPPER + 8:UPPER + 8 + 321]
    for colour in (pc.GREEN, pc.OLIVE):
        assert not (lower == np.array(colour, np.uint8)).all(axis=2).any()


def test_evalnoise_and_evalrand_figures(corpus, monkeypatch, capsys):
    from f2cnn_amd.scripts.CNN import Evaluating
    root, wav, bare, model = corpus
    monkeypatch.chdir(root)
    Evaluating.EvaluateWithNoise(wav, SNRdB=10, model=model, hop=160, rng=np.random.default_rng(5), figure=True, figure_width=64)
    assert read_png(os.path.join("graphs", "FallingOrRising", "DR1.FSYN0.SA110dB.png")).shape == (UPPER + 341, 64, 3)
    assert "figure_track" in np.load(os.path.join("OutputWavFiles", "addedNoise", "DR1.FSYN0.SA110dB.F2CNN.npz"))
    singles = {}
    for file in (wav, bare):
        Evaluating.EvaluateOneWavFile(file, hop=160, model=model, figure=True, figure_width=64)
        singles[file] = dict(np.load(os.path.splitext(file)[0] + ".F2CNN.npz"))
        os.remove(os.path.join("graphs", "FallingOrRising", os.path.splitext(os.path.basename(file))[0] + ".png"))
    results = Evaluating.EvaluateRandom(model=model, hop=160, figure=True, figure_width=64)          # both files: one batched call
    assert sorted(os.path.abspath(str(f)) for f in results) == sorted([wav, bare])     # (named as the glob finds them)
    for file in (wav, bare):
        got = dict(np.load(os.path.splitext(file)[0] + ".F2CNN.npz"))
        assert sorted(got) == sorted(singles[file])
        for key in got:
            assert np.array_equal(bits(got[key]), bits(singles[file][key])), (file, key)
        stem = os.path.splitext(os.path.basename(file))[0]
        assert read_png(os.path.join("graphs", "FallingOrRising", stem + ".png")).shape == (UPPER + 341, 64, 3)
