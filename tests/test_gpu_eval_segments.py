"""f2_eval_segments_batch: the strided evaluation with the decoder behind it on the device. Every output equals, byte for byte, the
strided call and the three stage calls on its scores; the path equals the sequential referee run on the device's own emissions;
host and device memory agree; outputs are optional; argument errors come in the stated order with nothing written. Then the command:
`cnn eval --segments` on a temporary file, its keys and its two tables."""
import os

import numpy as np
import pytest

import f2cnn_oracle as orc
import label_referee as lr
import segments_referee as ref
from devmem import Arena
from f2cnn_amd import _lib, segments
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

C, RADIUS, STEP = 128, 5, 160
LENGTHS = (4000, 1700, 16000, 0, 5000)          # 1700: no window; 16000 at hop 1: 14 tiles; an empty utterance
H, D = _lib.MEM_HOST, _lib.MEM_DEVICE


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def setup():
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))
    waves = [orc.synth_utterance(60 + i, n) for i, n in enumerate(LENGTHS)]
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    return coefs, np.concatenate(waves).astype(np.int16), offsets, F2CNNModel(orc.glorot_weights(7))


def intervals():
    """a set per utterance (R = B): touching phonemes over the third utterance, none for the others but one"""
    sets = [[[0, 2000], [2000, 4000]], [], [[0, 1000], [1000, 7000], [7000, 7000], [7000, 16000]], [[0, 10]], []]
    ivo = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return ivo, np.array([iv for s in sets for iv in s], np.int64).reshape(-1, 2)


def fused(ctx, setup, hop, scale, penalty, mem=H, want=("scores", "labels", "path", "emissions", "runs", "tally")):
    coefs, flat, offsets, model = setup
    B = len(LENGTHS)
    n = sum(_lib.strided_window_count(int(m), RADIUS, STEP, hop) for m in LENGTHS)
    ivo, ivb = intervals()
    shapes = dict(scores=(np.float32, 2 * n), labels=(np.uint8, n), path=(np.uint8, n), emissions=(np.int32, n), runs=(np.int64, 4 * n),
                  tally=(np.int64, 4 * int(ivo[-1])))
    if mem == H:
        out = {k: np.full(shapes[k][1], 0x5A, shapes[k][0]) for k in want}
        wo, value, ro = ctx.eval_segments_batch(model.handle(ctx), flat, _lib.WAVE_I16, offsets, coefs, B, C, True, 50.0, _lib.FFT_F32, RADIUS,
                                                STEP, hop, scale, penalty, ivo, ivb, *[out.get(k) for k in shapes], H)
    else:
        with Arena(ctx) as a:
            a.region("wave", np.int16, len(flat), misalign=1, role="in")
            for i, k in enumerate(want):
                a.region(k, shapes[k][0], shapes[k][1], misalign=1 + 2 * (i % 2), role="out")
            a.upload("wave", flat)
            wo, value, ro = ctx.eval_segments_batch(model.handle(ctx), a.ptr("wave"), _lib.WAVE_I16, offsets, coefs, B, C, True, 50.0,
                                                    _lib.FFT_F32, RADIUS, STEP, hop, scale, penalty, ivo, ivb,
                                                    *[a.ptr(k) if k in want else None for k in shapes], D)
            ctx.synchronize()
            a.check()
            out = {k: a.download(k).copy() for k in want}
    assert wo[-1] == n
    if "runs" in out:
        out["runs"] = out["runs"][:4 * int(ro[-1])]
    return out, wo, value, ro


_staged = {}


def staged(ctx, setup, hop, scale, penalty):
    """the strided call and the three stage calls, each on what the one before returned"""
    key = (hop, scale, penalty)
    if key not in _staged:
        coefs, flat, offsets, model = setup
        n = sum(_lib.strided_window_count(int(m), RADIUS, STEP, hop) for m in LENGTHS)
        out = dict(scores=np.empty(2 * n, np.float32), labels=np.empty(n, np.uint8), path=np.empty(n, np.uint8), emissions=np.empty(n, np.int32))
        wo = ctx.eval_batch_strided(model.handle(ctx), flat, _lib.WAVE_I16, offsets, coefs, len(LENGTHS), C, True, 50.0, _lib.FFT_F32,
                                    RADIUS, STEP, hop, out["scores"], out["labels"], H)
        value = ctx.decision_path(out["scores"], wo, scale, penalty, out["path"], H, emissions=out["emissions"])
        runs = np.empty(4 * n, np.int64)
        ro = ctx.decision_runs(out["path"], out["emissions"], wo, runs, n, H)
        out["runs"] = runs[:4 * int(ro[-1])]
        ivo, ivb = intervals()
        out["tally"] = ctx.interval_tally(out["labels"], out["path"], out["emissions"], wo, ivo, ivb, RADIUS * STEP, hop,
                                          np.empty(4 * int(ivo[-1]), np.int64), H)
        _staged[key] = (out, wo, value, ro)
    return _staged[key]


@pytest.mark.parametrize("hop", [1, 160])
@pytest.mark.parametrize("mem", [H, D])
def test_fused_call_equals_the_strided_call_and_the_three_stages(ctx, setup, hop, mem):
    scale, penalty = segments.Quantise(hop, STEP, 16000)
    want, wo_s, value_s, ro_s = staged(ctx, setup, hop, scale, penalty)
    got, wo, value, ro = fused(ctx, setup, hop, scale, penalty, mem)
    assert np.array_equal(wo, wo_s) and np.array_equal(value, value_s) and np.array_equal(ro, ro_s)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    # the path is the referee's on the device's own emissions; the runs and the tally are the referee's on that path
    path, val = ref.decision_path(got["emissions"], wo, penalty)
    assert np.array_equal(path, got["path"]) and np.array_equal(val, value)
    ro_r, runs_r = ref.decision_runs(got["path"], got["emissions"], wo)
    assert np.array_equal(ro_r, ro) and np.array_equal(runs_r.reshape(-1), got["runs"])
    ivo, ivb = intervals()
    assert np.array_equal(ref.interval_tally(got["labels"], got["path"], got["emissions"], wo, ivo, ivb, RADIUS * STEP, hop).reshape(-1),
                          got["tally"])
    assert int(ro[-1]) < int(wo[-1])            # smoothing joins rows


def test_every_output_is_optional(ctx, setup):
    hop = 160
    scale, penalty = segments.Quantise(hop, STEP, 16000)
    want = staged(ctx, setup, hop, scale, penalty)[0]
    for subset in (("tally",), ("runs",), ("path",), ("scores", "labels")):
        for mem in (H, D):
            got = fused(ctx, setup, hop, scale, penalty, mem, want=subset)[0]
            for k in subset:
                assert got[k].tobytes() == want[k].tobytes(), (subset, mem, k)


def test_argument_errors_in_their_order(ctx, setup):
    coefs, flat, offsets, model = setup
    B, hop = len(LENGTHS), 160
    n = sum(_lib.strided_window_count(int(m), RADIUS, STEP, hop) for m in LENGTHS)
    ivo, ivb = intervals()
    outs = dict(sc=np.full(2 * n, 5, np.float32), lb=np.full(n, 5, np.uint8), wo=np.full(B + 1, -9, np.int64), path=np.full(n, 5, np.uint8),
                q=np.full(n, 5, np.int32), value=np.full(B, -9, np.int64), ro=np.full(B + 1, -9, np.int64), runs=np.full(4 * n, -9, np.int64),
                tally=np.full(4 * int(ivo[-1]), -9, np.int64))
    before = {k: v.copy() for k, v in outs.items()}

    def call(hop=hop, scale=65536.0, penalty=100, ivo=ivo, ivb=ivb, R=B, C_=C, wave=flat):
        p = lambda x: None if x is None else x.ctypes.data
        return ctx.lib.f2_eval_segments_batch(ctx.handle, model.handle(ctx), p(wave), _lib.WAVE_I16, p(offsets), p(coefs), B, C_, 1, 50.0,
                                              _lib.FFT_F32, RADIUS, STEP, hop, scale, penalty, p(ivo), p(ivb), R, *[p(v) for v in outs.values()], H)

    inv, uns = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    assert call(hop=0, scale=-1.0) == inv and "hop" in ctx.lib.f2_last_error(ctx.handle).decode()          # the strided call's checks first
    assert call(C_=64, penalty=-1) == inv and "network" in ctx.lib.f2_last_error(ctx.handle).decode()
    assert call(wave=None, scale=0.0) == inv and "wave" in ctx.lib.f2_last_error(ctx.handle).decode()
    assert call(scale=0.0, R=B - 1) == inv and "logit_scale" in ctx.lib.f2_last_error(ctx.handle).decode()   # then path, then tally
    assert call(penalty=(1 << 40) + 1) == uns and call(scale=float(2 ** 21)) == uns
    assert call(ivo=None) == inv and call(R=B - 1) == inv
    bad = ivb.copy()
    bad[1, 0] = 1999
    assert call(ivb=bad) == inv
    for k in outs:
        assert outs[k].tobytes() == before[k].tobytes(), k
    assert call() == _lib.F2_OK and outs["wo"][-1] == n and (outs["path"] <= 1).all()


# ---- the command --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from f2cnn_amd import config
    root = tmp_path_factory.mktemp("segmentscorpus")
    config.write_default(str(root / "configF2CNN.conf"))
    folder = root / "resources" / "f2cnn" / "TEST"
    os.makedirs(folder)
    wav = lr.write_labelled_file(folder, lambda n: orc.synth_utterance(21, n))
    with open(os.path.splitext(wav)[0] + ".PHN", "w") as f:
        f.write("0 3000 h#\n3000 9000 aa\n9000 14000 t\n14000 19200 aa\n")
    F2CNNModel(orc.glorot_weights(7)).save(str(root / "model.npz"))
    return root, wav


def test_cnn_eval_segments_command(corpus, monkeypatch, capsys):
    from f2cnn_amd import cli
    root, wav = corpus
    monkeypatch.chdir(root)
    npz = os.path.splitext(wav)[0] + ".F2CNN.npz"
    assert cli.main(["cnn", "eval", "-f", wav, "-m", "model.npz", "--hop", "frame"]) == 0
    plain = dict(np.load(npz))
    capsys.readouterr()
    assert cli.main(["cnn", "eval", "-f", wav, "-m", "model.npz", "--hop", "frame", "--segments", "--accuracy", "centre"]) == 0
    printed = capsys.readouterr().out
    got = dict(np.load(npz))
    keys = ["path", "runs", "run_offsets", "value", "logit_scale", "penalty", "phoneme_names", "phoneme_tally"]
    assert all("segments_" + k in got for k in keys)
    assert got["scores"].tobytes() == plain["scores"].tobytes() and np.array_equal(got["labels"], plain["labels"])
    n = len(got["labels"])
    runs = got["segments_runs"]
    assert got["segments_path"].shape == (n,) and runs[:, 1].sum() == n and got["segments_run_offsets"].tolist() == [0, len(runs)]
    assert got["segments_logit_scale"] == 65536.0 and got["segments_penalty"] == round(65536 * np.log(2.0))
    assert got["segments_phoneme_names"].tolist() == ["h#", "aa", "t"] and got["segments_phoneme_tally"][:, 0].sum() == n
    assert got["segments_phoneme_tally"][:, 2].sum() == int(got["segments_path"].sum())
    lines = printed.splitlines()
    at = next(i for i, line in enumerate(lines) if "transitions ({} runs)".format(len(runs)) in line)
    rows = [line.split("\t")[2:] for line in lines[at + 2:at + 2 + len(runs)]]
    assert [r[3] for r in rows] == ["rising" if r else "falling" for r in runs[:, 2]]
    assert all(float(r[2]) == 10.0 * m for r, m in zip(rows, runs[:, 1])) and all(r[5] for r in rows)       # durations in ms; phonemes named
    at = next(i for i, line in enumerate(lines) if "decisions per phoneme" in line)
    table = [line.split("\t")[2:] for line in lines[at + 2:at + 5]]
    assert [t[0] for t in table] == ["h#", "aa", "t"] and [int(t[1]) for t in table] == got["segments_phoneme_tally"][:, 0].tolist()
    assert sum("accuracy against the VTR labels" in line for line in lines) == 2 and "(smoothed)" in printed
    assert "segments_confusion" in got and "confusion" in got
    # beside a figure the three stage calls run on the figure call's scores: the same keys, the same bytes
    assert cli.main(["cnn", "eval", "-f", wav, "-m", "model.npz", "--hop", "frame", "--segments", "--figure", "--figure-width", "64"]) == 0
    beside = dict(np.load(npz))
    for k in keys:
        assert beside["segments_" + k].tobytes() == got["segments_" + k].tobytes(), k


def test_evalnoise_and_evalrand_take_segments(corpus, monkeypatch, capsys):
    from f2cnn_amd.scripts.CNN import Evaluating
    root, wav = corpus
    monkeypatch.chdir(root)
    model = F2CNNModel(orc.glorot_weights(7))
    Evaluating.EvaluateOneWavFile(wav, hop=160, model=model, segments=True)
    single = dict(np.load(os.path.splitext(wav)[0] + ".F2CNN.npz"))
    Evaluating.EvaluateWithNoise(wav, SNRdB=10, model=model, hop=160, rng=np.random.default_rng(5), segments=dict(dwell_ms=50.0))
    noisy = dict(np.load(os.path.join("OutputWavFiles", "addedNoise", "DR1.FSYN0.SA110dB.F2CNN.npz")))
    assert noisy["segments_penalty"] == round(65536 * np.log(4.0)) and noisy["segments_runs"][:, 1].sum() == len(noisy["labels"])
    assert noisy["segments_phoneme_names"].tolist() == ["h#", "aa", "t"]           # the clean file's .PHN
    capsys.readouterr()
    results = Evaluating.EvaluateRandom(model=model, hop=160, segments=True, accuracy="centre")
    printed = capsys.readouterr().out
    assert len(results) == 1 and "(smoothed)" in printed and "decisions per phoneme" in printed
    again = dict(np.load(os.path.splitext(wav)[0] + ".F2CNN.npz"))
    for k in single:
        if k.startswith("segments_"):
            assert again[k].tobytes() == single[k].tobytes(), k
    assert "segments_confusion" in again


def test_evalrand_mixed_group_with_options_equals_eval(tmp_path, monkeypatch, capsys):
    """a group of two rates goes through the batch pass file by file: with segments and a figure every file's .npz is, byte for byte,
    the one `cnn eval` writes for it alone. 4000 samples at 16 kHz and 2000 at 8 kHz (STEP 80): 14 and 7 rows at the hop."""
    from scipy.io import wavfile
    from f2cnn_amd import config, wavio
    from f2cnn_amd.scripts.CNN import Evaluating
    monkeypatch.chdir(tmp_path)
    config.write_default(str(tmp_path / "configF2CNN.conf"))
    folder = tmp_path / "resources" / "f2cnn" / "TEST"
    os.makedirs(folder)
    files = [os.path.join("resources", "f2cnn", "TEST", name) for name in ("WIDE.WAV", "NARROW.WAV")]
    wavio.write_sphere(files[0], 16000, orc.synth_utterance(31, 4000))
    wavfile.write(files[1], 8000, orc.synth_utterance(32, 2000).astype(np.int16))
    model = F2CNNModel(orc.glorot_weights(7))
    keywords = dict(model=model, hop=160, segments=True, figure=True, figure_width=64)
    alone = {}
    for file in files:
        Evaluating.EvaluateOneWavFile(file, **keywords)
        alone[file] = dict(np.load(os.path.splitext(file)[0] + ".F2CNN.npz"))
        os.remove(os.path.splitext(file)[0] + ".F2CNN.npz")
    results = Evaluating.EvaluateRandom(**keywords)
    assert sorted(results) == sorted(files)
    for file, rows in zip(files, (14, 7)):
        grouped = dict(np.load(os.path.splitext(file)[0] + ".F2CNN.npz"))
        assert set(grouped) == set(alone[file]) and len(grouped["labels"]) == rows and "segments_path" in grouped and "figure_track" in grouped
        for key, value in alone[file].items():
            assert grouped[key].dtype == value.dtype and grouped[key].tobytes() == value.tobytes(), (file, key)
