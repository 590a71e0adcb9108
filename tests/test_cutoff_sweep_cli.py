"""`cnn lpfsweep`: the parts that need no GPU - the command line takes the new command and `--cutoffs`, refuses what the sweep
does not do, leaves `cnn noisesweep` and its messages as they were; the two C entry points are declared and bound; and
EvaluateCutoffSweep groups its files and writes its .npz, held against a stub context that stands in for the device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, cli


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_parser_takes_the_sweep():
    args = cli.build_parser().parse_args(["cnn", "lpfsweep", "--file", "a.WAV", "--cutoffs", "5,10,20,50,100", "--hop", "frame"])
    assert args.cnn_command == "lpfsweep" and args.file == "a.WAV" and args.hop == "frame"
    assert args.cutoffs == [5.0, 10.0, 20.0, 50.0, 100.0]
    assert cli.build_parser().parse_args(["cnn", "lpfsweep", "-f", "a.WAV", "--cutoffs", "0.5"]).cutoffs == [0.5]
    assert cli.build_parser().parse_args(["cnn", "lpfsweep", "-f", "a.WAV", "--cutoffs", "7999.5,2.5e1"]).cutoffs == [7999.5, 25.0]
    assert "lpfsweep" in cli.CNN and "lpfsweep" in cli.__doc__ and "--cutoffs" in cli.__doc__


@pytest.mark.parametrize("bad", ["20,x", "", "20,,10", "nan", "inf,3", "0", "8000", "-5", "50,0", "50,9000"])
def test_parser_refuses_a_malformed_list(bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "lpfsweep", "--file", "a.WAV", "--cutoffs=" + bad])
    assert e.value.code == 2
    assert "--cutoffs" in capsys.readouterr().err


@pytest.fixture
def no_evaluation(monkeypatch):
    """any evaluation the command line would start is recorded, not run"""
    from f2cnn_amd.scripts.CNN import Evaluating
    seen = []
    for name in ("EvaluateCutoffSweep", "EvaluateNoiseSweep", "EvaluateOneWavFile", "EvaluateWithNoise", "EvaluateRandom"):
        monkeypatch.setattr(Evaluating, name, lambda *a, _name=name, **kw: seen.append((_name, a, kw)))
    return seen


@pytest.mark.parametrize("extra,word", [(["--lpf", "50"], "--lpf"), (["--figure"], "--figure"), (["--occlusion"], "--occlusion"),
                                        (["--occlusion", "8:4"], "--occlusion")])
def test_sweep_refuses_lpf_figure_and_occlusion(no_evaluation, capsys, extra, word):
    assert cli.main(["cnn", "lpfsweep", "--file", "a.WAV", "--cutoffs", "5,50"] + extra) == 1
    out = capsys.readouterr().out
    assert word in out and "lpfsweep" in out and no_evaluation == []


def test_sweep_needs_a_file_and_cutoffs(no_evaluation, capsys):
    assert cli.main(["cnn", "lpfsweep", "--cutoffs", "5,50"]) == 1
    assert capsys.readouterr().out == "Please use --file or -f to give input file\n"
    assert cli.main(["cnn", "lpfsweep", "--file", "a.WAV"]) == 1
    assert "--cutoffs" in capsys.readouterr().out
    assert no_evaluation == []


def test_sweep_hands_its_options_down(no_evaluation, monkeypatch, tmp_path):
    from f2cnn_amd import config
    monkeypatch.chdir(tmp_path)
    config.write_default()
    assert cli.main(["cnn", "lpfsweep", "--file", "a.WAV", "--cutoffs", "5,50", "--hop", "frame", "--accuracy", "--resample", "--model",
                     "m.npz"]) == 0
    (name, a, kw), = no_evaluation
    assert name == "EvaluateCutoffSweep" and a == (["a.WAV"], [5.0, 50.0])
    assert kw == dict(hop=config.F2Config().step, accuracy="reference", resample=True, model="m.npz")


def test_noisesweep_messages_are_unchanged(no_evaluation, capsys):
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3", "--figure"]) == 1
    assert capsys.readouterr().out == "--figure is not supported by noisesweep (use evalnoise --figure for one level)\n"
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3", "--occlusion"]) == 1
    assert capsys.readouterr().out == "--occlusion is not supported by noisesweep (use evalnoise --occlusion for one level)\n"
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV"]) == 1
    assert capsys.readouterr().out == "Please use --snrs to give the noise levels, e.g. --snrs 20,10,0,-3\n"
    assert cli.main(["cnn", "noisesweep", "--snrs", "3"]) == 1
    assert capsys.readouterr().out == "Please use --file or -f to give input file\n"
    assert no_evaluation == []
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3,0", "--lpf", "50"]) == 0     # --lpf stays noisesweep's
    (name, a, kw), = no_evaluation
    assert name == "EvaluateNoiseSweep" and a == (["a.WAV"], [3.0, 0.0]) and kw == dict(seed=0, save_wavs=False, LPF=True, CUTOFF=50)


def test_other_commands_parse_as_before():
    args = vars(cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3"]))
    assert "cutoffs" not in args


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+f2_lowpass_levels\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_lowpass_levels is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["f2_ctx* ctx", "const double* env", "const int64_t* offsets", "int B", "int C", "const double* cutoff_hz", "int K",
                      "double* levels", "int mem_space"]
    res, args = _lib.SIGNATURES["f2_lowpass_levels"]
    assert res is ctypes.c_int and len(args) == len(params)
    m = re.search(r"\bint\s+f2_eval_cutoff_sweep\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_eval_cutoff_sweep is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert len(params) == 20
    assert params[8:14] == ["int fft_precision", "int radius", "int step", "int hop", "const double* cutoff_hz", "int K"]
    assert params[14:] == ["double* env_levels_or_null", "float* scores_or_null", "uint8_t* labels_or_null",
                           "int64_t* window_offsets_or_null", "int64_t* stats_or_null", "int mem_space"]
    res, args = _lib.SIGNATURES["f2_eval_cutoff_sweep"]
    assert res is ctypes.c_int and len(args) == len(params)
    # the binding is f2_eval_batch_strided's without lpf / cutoff_hz, then the cutoffs, then the outputs
    base = _lib.SIGNATURES["f2_eval_batch_strided"][1]
    assert args[:8] == base[:8] and args[8:12] == base[10:14] and args[12:14] == [ctypes.c_void_p, ctypes.c_int]
    assert args[14:] == [ctypes.c_void_p] * 5 + [ctypes.c_int]
    for word in ("tan(pi * cutoff / 16000)", "b0 = k / (1 + k)", "a1 = (k - 1) / (k + 1)", "EnvelopeExtraction.py:39-67"):
        assert word in text, word
    assert "cutoffs" in inspect.signature(_lib.Context.eval_cutoff_sweep).parameters
    assert "cutoffs" in inspect.signature(_lib.Context.lowpass_levels).parameters
    from f2cnn_amd.scripts.CNN import Evaluating
    p = inspect.signature(Evaluating.EvaluateCutoffSweep).parameters
    assert list(p) == ["files", "cutoffs", "hop", "model", "ctx", "accuracy", "resample"]
    assert (p["hop"].default, p["model"].default, p["ctx"].default, p["accuracy"].default, p["resample"].default) == \
        (None, "last_trained_model", None, None, False)


# ---- EvaluateCutoffSweep against a stub context -------------------------------------------------------------------------------------------
RADIUS, STEP, R = 5, 160, 11


class StubContext:
    """Stands in for the device: labels window j of level l of file b as (j + l + b) % 2 == 0 and counts like the tally."""

    def __init__(self):
        self.calls = []

    def cnn_create(self, tensors, rows, channels):
        return 1

    def eval_cutoff_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, precision, radius, step, hop, cutoffs, env_levels,
                          scores, labels, mem_space):
        K = len(cutoffs)
        lengths = np.diff(offsets)
        self.calls.append(dict(B=B, lengths=lengths.tolist(), dtype=wave_dtype, Cn=Cn, hop=hop, cutoffs=list(cutoffs), step=step))
        assert handle == 1 and env_levels is None and mem_space == _lib.MEM_HOST and wave.shape[0] == offsets[-1]
        per = [_lib.strided_window_count(int(n), radius, step, hop) for n in lengths] * (K + 1)
        wo = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        assert labels.shape == (wo[-1],) and scores.shape == (wo[-1], 2)
        for u in range((K + 1) * B):
            l, b = divmod(u, B)
            labels[wo[u]:wo[u + 1]] = (np.arange(per[u]) + l + b) % 2 == 0
        scores[:, 1] = 0.25 + 0.5 * labels
        scores[:, 0] = 1 - scores[:, 1]
        stats = np.zeros(((K + 1) * B, 2), np.int64)
        for u in range((K + 1) * B):
            mine, ref = labels[wo[u]:wo[u + 1]], labels[wo[K * B + u % B]:wo[K * B + u % B + 1]]
            stats[u] = mine.sum(), (mine == ref).sum()
        return wo, stats


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    from f2cnn_amd import config
    monkeypatch.chdir(tmp_path)
    config.write_default()
    return tmp_path


def write_wavs(workdir, lengths, rate=16000, dtype=np.int16):
    from scipy.io import wavfile
    files = []
    rng = np.random.default_rng(3)
    for i, n in enumerate(lengths):
        path = str(workdir / "F{}_{}_{}.WAV".format(rate, np.dtype(dtype).name, i))
        wavfile.write(path, rate, (rng.standard_normal(n) * 3000).astype(dtype))
        files.append(path)
    return files


def test_evaluate_cutoff_sweep_groups_and_writes(workdir, capsys):
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    lengths = [2000 + 7 * i for i in range(18)]
    files = write_wavs(workdir, lengths) + write_wavs(workdir, [2500], rate=8000)
    stub = StubContext()
    res = Evaluating.EvaluateCutoffSweep(files, [5, 50.5], hop=160, model=F2CNNModel.glorot(7), ctx=stub)
    # one rate per pass, 16 files at the most
    assert [c["B"] for c in stub.calls] == [16, 2, 1]
    assert stub.calls[0]["lengths"] == lengths[:16] and stub.calls[1]["lengths"] == lengths[16:] and stub.calls[2]["lengths"] == [2500]
    assert [c["step"] for c in stub.calls] == [160, 160, 80] and all(c["cutoffs"] == [5.0, 50.5] and c["hop"] == 160 for c in stub.calls)
    assert list(res) == files
    K = 2
    expected = ""
    for i, file in enumerate(files):
        out = os.path.splitext(file)[0] + ".lpfsweep.npz"
        archive = np.load(out)
        assert list(archive.files) == list(res[file]) == ["cutoff_hz", "windows", "rising", "agree", "agreement", "hop", "timepoints",
                                                          "scores", "labels_0", "labels_1", "labels_nolpf"]
        n = _lib.strided_window_count(lengths[i], RADIUS, STEP, 160) if i < 18 else _lib.strided_window_count(2500, RADIUS, 80, 160)
        expected += "File:\t\t{}\n".format(file)
        for l, name in enumerate(("5Hz", "50.5Hz", "nolpf")):
            rising = ((np.arange(n) + l + (i % 16 if i < 18 else 0)) % 2 == 0).sum()
            expected += "\tcutoff {:>8}\t{} windows\t{} rising\tagreement with nolpf {:.4f}\n".format(name, n, rising, (1.0, 0.0, 1.0)[l])
        expected += "\t\t{}\tdone ! -> {}\n".format(file, out)
        if i >= 18:
            continue
        saved = dict(archive)
        b = i % 16
        assert saved["windows"].tolist() == [n] * (K + 1) and int(saved["hop"]) == 160 and saved["cutoff_hz"].tolist() == [5.0, 50.5]
        assert saved["scores"].shape == (K + 1, n, 2) and saved["scores"].dtype == np.float32
        assert np.array_equal(saved["timepoints"], RADIUS * STEP + 160 * np.arange(n))
        for l, key in enumerate(("labels_0", "labels_1", "labels_nolpf")):
            assert np.array_equal(saved[key], (np.arange(n) + l + b) % 2 == 0), (i, key)
            assert saved["rising"][l] == saved[key].sum() and saved["agree"][l] == (saved[key] == saved["labels_nolpf"]).sum()
            assert np.array_equal(saved["scores"][l][:, 1], np.float32(0.25) + np.float32(0.5) * saved[key])
            assert np.array_equal(res[file][key], saved[key])
        assert saved["agreement"].tolist() == [1.0, 0.0, 1.0]
    printed = capsys.readouterr().out
    assert printed.count("agreement with nolpf") == 19 * (K + 1) and "50.5Hz" in printed and "nolpf" in printed
    assert printed.count("File:") == 19
    assert printed == expected


def test_groups_shrink_where_the_levels_would_not_fit():
    from f2cnn_amd.scripts.CNN import Evaluating
    members = [("f%d" % i, np.zeros(n, np.int16)) for i, n in enumerate((100, 100, 100, 500, 50))]
    K, Cn = 1, 2
    limit = (K + 1) * Cn * 200 * 8
    groups = list(Evaluating._cutoff_groups(members, K, Cn, limit=limit))
    assert [[f for f, _ in g] for g in groups] == [["f0", "f1"], ["f2"], ["f3"], ["f4"]]       # a file beyond the limit: alone
    assert [len(g) for g in Evaluating._cutoff_groups(members * 4, K, Cn, batch=16)] == [16, 4]
    assert Evaluating.LEVELS_LIMIT == 8 << 30


@pytest.mark.parametrize("bad", [[], [0], [8000], [float("nan")], [50, -1]])
def test_bad_cutoffs_are_refused_before_anything_is_read(bad):
    from f2cnn_amd.scripts.CNN import Evaluating
    with pytest.raises(ValueError, match="cutoff"):
        Evaluating.EvaluateCutoffSweep(["does-not-exist.WAV"], bad, ctx=StubContext())
