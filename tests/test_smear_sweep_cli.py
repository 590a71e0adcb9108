"""`cnn smearsweep`: the parts that need no GPU - the command line takes the new command with `--spreads` and `--bands`, refuses
what the sweep does not do, leaves the other sweeps and their messages as they were; the two C entry points are declared and
bound, the tile constants of the binding are the kernel's; smear.SmearMatrix and smear.BandMatrix; and EvaluateSmearSweep groups
its files and writes its .npz, held against a stub context that stands in for the device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, cli, smear
from f2cnn_amd.gammatone import filters


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_parser_takes_the_sweep():
    args = cli.build_parser().parse_args(["cnn", "smearsweep", "--file", "a.WAV", "--spreads", "0.5,1,2,4", "--bands", "32,16,8", "--hop",
                                          "frame"])
    assert args.cnn_command == "smearsweep" and args.file == "a.WAV" and args.hop == "frame"
    assert args.spreads == [0.5, 1.0, 2.0, 4.0] and args.bands == [32, 16, 8]
    only = cli.build_parser().parse_args(["cnn", "smearsweep", "-f", "a.WAV", "--bands", "8"])
    assert only.bands == [8] and "spreads" not in vars(only)
    only = cli.build_parser().parse_args(["cnn", "smearsweep", "-f", "a.WAV", "--spreads", "2.5e-1"])
    assert only.spreads == [0.25] and "bands" not in vars(only)
    assert "smearsweep" in cli.CNN and "smearsweep" in cli.SWEEPS and "smearsweep" in cli.__doc__
    assert "--spreads" in cli.__doc__ and "--bands" in cli.__doc__


@pytest.mark.parametrize("option,bad", [("--spreads", ""), ("--spreads", "nan"), ("--spreads", "0"), ("--spreads", "-1"), ("--spreads", "1,,2"),
                                        ("--spreads", "1,x"), ("--spreads", "inf"), ("--bands", ""), ("--bands", "nan"), ("--bands", "0"),
                                        ("--bands", "-1"), ("--bands", "1.5"), ("--bands", "8,,4"), ("--bands", "8,x")])
def test_parser_refuses_a_malformed_list(option, bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "smearsweep", "--file", "a.WAV", option + "=" + bad])
    assert e.value.code == 2
    assert option in capsys.readouterr().err


@pytest.fixture
def no_evaluation(monkeypatch):
    """any evaluation the command line would start is recorded, not run"""
    from f2cnn_amd.scripts.CNN import Evaluating
    seen = []
    for name in ("EvaluateSmearSweep", "EvaluateCutoffSweep", "EvaluateNoiseSweep", "EvaluateReverbSweep", "EvaluateOneWavFile",
                 "EvaluateWithNoise", "EvaluateRandom"):
        monkeypatch.setattr(Evaluating, name, lambda *a, _name=name, **kw: seen.append((_name, a, kw)))
    return seen


@pytest.mark.parametrize("extra,word", [(["--figure"], "--figure"), (["--occlusion"], "--occlusion"), (["--occlusion", "8:4"], "--occlusion")])
def test_sweep_refuses_figure_and_occlusion(no_evaluation, capsys, extra, word):
    assert cli.main(["cnn", "smearsweep", "--file", "a.WAV", "--spreads", "1"] + extra) == 1
    assert capsys.readouterr().out == "{} is not supported by smearsweep (use eval {} for the sharp level)\n".format(word, word)
    assert no_evaluation == []


def test_sweep_needs_a_file_and_a_level(no_evaluation, capsys):
    assert cli.main(["cnn", "smearsweep", "--spreads", "1"]) == 1
    assert capsys.readouterr().out == "Please use --file or -f to give input file\n"
    assert cli.main(["cnn", "smearsweep", "--file", "a.WAV"]) == 1
    out = capsys.readouterr().out
    assert "--spreads" in out and "--bands" in out
    assert no_evaluation == []


def test_sweep_hands_its_options_down(no_evaluation, monkeypatch, tmp_path):
    from f2cnn_amd import config
    monkeypatch.chdir(tmp_path)
    config.write_default()
    assert cli.main(["cnn", "smearsweep", "--file", "a.WAV", "--spreads", "0.5,2", "--bands", "16", "--hop", "frame", "--accuracy", "--resample",
                     "--model", "m.npz", "--lpf", "50"]) == 0
    (name, a, kw), = no_evaluation
    assert name == "EvaluateSmearSweep" and a == (["a.WAV"],)
    assert kw == dict(spreads=[0.5, 2.0], bands=[16], hop=config.F2Config().step, accuracy="reference", resample=True, model="m.npz", LPF=True,
                      CUTOFF=50)
    del no_evaluation[:]
    assert cli.main(["cnn", "smearsweep", "--file", "a.WAV", "--bands", "8,4", "--hop", "7"]) == 0
    (name, a, kw), = no_evaluation
    assert a == (["a.WAV"],) and kw == dict(spreads=(), bands=[8, 4], hop=7)


def test_the_other_sweeps_messages_are_unchanged(no_evaluation, capsys):
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3", "--figure"]) == 1
    assert capsys.readouterr().out == "--figure is not supported by noisesweep (use evalnoise --figure for one level)\n"
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV"]) == 1
    assert capsys.readouterr().out == "Please use --snrs to give the noise levels, e.g. --snrs 20,10,0,-3\n"
    assert cli.main(["cnn", "lpfsweep", "--file", "a.WAV", "--cutoffs", "5", "--lpf", "50"]) == 1
    assert capsys.readouterr().out == "--lpf is not supported by lpfsweep (the cutoffs come from --cutoffs; the unfiltered level is always there)\n"
    assert cli.main(["cnn", "lpfsweep", "--file", "a.WAV"]) == 1
    assert capsys.readouterr().out == "Please use --cutoffs to give the envelope cutoffs in Hz, e.g. --cutoffs 5,10,20,50,100\n"
    assert cli.main(["cnn", "reverbsweep", "--file", "a.WAV", "--t60", "0.2", "--occlusion"]) == 1
    assert capsys.readouterr().out == "--occlusion is not supported by reverbsweep (use eval --occlusion on a WAV written with --save-wavs)\n"
    assert no_evaluation == []


def test_other_commands_parse_as_before():
    for command, option, value in (("noisesweep", "--snrs", "3"), ("lpfsweep", "--cutoffs", "5"), ("reverbsweep", "--t60", "0.2")):
        args = vars(cli.build_parser().parse_args(["cnn", command, "--file", "a.WAV", option, value]))
        assert "spreads" not in args and "bands" not in args
    assert "spreads" not in vars(cli.build_parser().parse_args(["cnn", "eval", "--file", "a.WAV"]))


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+f2_channel_mix_levels\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_channel_mix_levels is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["f2_ctx* ctx", "const double* env", "const int64_t* offsets", "int B", "int C", "const double* mix", "int K",
                      "double* levels", "int mem_space"]
    res, args = _lib.SIGNATURES["f2_channel_mix_levels"]
    assert res is ctypes.c_int and len(args) == len(params) and args == _lib.SIGNATURES["f2_lowpass_levels"][1]
    m = re.search(r"\bint\s+f2_eval_smear_sweep\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_eval_smear_sweep is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["f2_ctx* ctx", "const f2_cnn* cnn", "const void* wave", "int wave_dtype", "const int64_t* offsets", "const double* coefs",
                      "int B", "int C", "int lpf", "double cutoff_hz", "int fft_precision", "int radius", "int step", "int hop",
                      "const double* mix", "int K", "double* env_levels_or_null", "float* scores_or_null", "uint8_t* labels_or_null",
                      "int64_t* window_offsets_or_null", "int64_t* stats_or_null", "int mem_space"]
    res, args = _lib.SIGNATURES["f2_eval_smear_sweep"]
    assert res is ctypes.c_int and len(args) == len(params)
    # the binding is f2_eval_batch_strided's up to the hop, then the matrices, then the outputs
    base = _lib.SIGNATURES["f2_eval_batch_strided"][1]
    assert args[:14] == base[:14] and args[14:16] == [ctypes.c_void_p, ctypes.c_int]
    assert args[16:] == [ctypes.c_void_p] * 5 + [ctypes.c_int]
    assert re.search(r"\bint\s+f2_version\s*\(", code) and "f2_version stays 114" in text
    for method in (_lib.Context.channel_mix_levels, _lib.Context.eval_smear_sweep):
        assert "mix" in inspect.signature(method).parameters
    from f2cnn_amd.scripts.CNN import Evaluating
    p = inspect.signature(Evaluating.EvaluateSmearSweep).parameters
    assert list(p) == ["files", "spreads", "bands", "hop", "LPF", "CUTOFF", "model", "ctx", "accuracy", "resample"]
    assert [p[k].default for k in list(p)[1:]] == [(), (), None, False, 50, "last_trained_model", None, None, False]


def test_tile_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "f2cnn_amd", "csrc", "f2_internal.h")).read()
    for name, value in (("F2_SMEAR_TILE_SAMPLES", _lib.SMEAR_TILE_SAMPLES), ("F2_SMEAR_TILE_CHANNELS", _lib.SMEAR_TILE_CHANNELS),
                        ("F2_SMEAR_MAX_CHANNELS", _lib.SMEAR_MAX_CHANNELS), ("F2_SMEAR_MAX_LEVELS", _lib.SMEAR_MAX_LEVELS)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", text)
        assert m and int(m.group(1)) == value, name
    assert smear.MAX_CHANNELS == _lib.SMEAR_MAX_CHANNELS


# ---- the matrices -------------------------------------------------------------------------------------------------------------------------
FREQS = filters.centre_freqs(16000, 128, 100)


def test_the_channels_are_a_quarter_erb_apart():
    e = smear.erb_number(FREQS)
    assert np.allclose(np.abs(np.diff(e)), 0.233, atol=5e-4) and abs(smear.channel_spacing(FREQS) - 0.233) < 5e-4
    assert smear.channel_spacing([1000.0]) == np.inf


@pytest.mark.parametrize("erbs", [0.25, 0.5, 1.0, 2.0, 4.0])
def test_smear_matrix(erbs):
    W = smear.SmearMatrix(FREQS, erbs)
    assert W.shape == (128, 128) and W.dtype == np.float64 and W.flags["C_CONTIGUOUS"] and (W >= 0).all()
    assert (np.abs(W.sum(axis=1) - 1.0) <= 2.0 ** -52).all()                       # rows sum to 1 within an ulp
    d = np.abs(smear.erb_number(FREQS)[:, None] - smear.erb_number(FREQS)[None, :])
    assert (W[d > 4 * erbs] == 0).all() and (W[d <= 4 * erbs] > 0).all()            # zeros exactly beyond 4 sigma
    for row in W:                                                                  # the supports are contiguous
        nz = np.flatnonzero(row)
        assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))
    assert np.array_equal(W.argmax(axis=1), np.arange(128))
    ratio = W[64, 65] / W[64, 64]
    assert abs(ratio - np.exp(-0.5 * (d[64, 65] / erbs) ** 2)) < 1e-15
    # ascending centre frequencies serve as well (a row sum taken in the other order: an ulp)
    assert np.allclose(smear.SmearMatrix(FREQS[::-1], erbs), W[::-1, ::-1], rtol=4 * 2.0 ** -52, atol=0)


def test_the_support_widths_of_the_cost_model():
    """the table of DESIGN.md, "Smear sweep": FMAs per sample column at 128 channels"""
    walked = [int((smear.SmearMatrix(FREQS, v) > 0).sum()) for v in (0.25, 0.5, 1, 2, 4)]
    assert walked == [1132, 2104, 4174, 7642, 12844]


def test_smear_matrix_is_the_identity_below_a_quarter_of_the_spacing():
    spacing = smear.channel_spacing(FREQS)
    assert np.array_equal(smear.SmearMatrix(FREQS, spacing / 4.001), np.eye(128))
    assert np.array_equal(smear.SmearMatrix(FREQS, 1e-9), np.eye(128))
    assert not np.array_equal(smear.SmearMatrix(FREQS, spacing / 3.9), np.eye(128))
    assert np.array_equal(smear.SmearMatrix([440.0], 3.0), np.eye(1))


@pytest.mark.parametrize("bad", [0, -1, float("nan"), float("inf"), -float("inf")])
def test_smear_matrix_refuses_a_bad_spread(bad):
    with pytest.raises(ValueError, match="spread"):
        smear.SmearMatrix(FREQS, bad)


def test_smear_matrix_refuses_bad_centre_frequencies():
    with pytest.raises(ValueError):
        smear.SmearMatrix([100.0, 200.0, 200.0], 1.0)
    with pytest.raises(ValueError):
        smear.SmearMatrix([100.0, 300.0, 200.0], 1.0)
    with pytest.raises(ValueError):
        smear.SmearMatrix(np.linspace(100, 8000, _lib.SMEAR_MAX_CHANNELS + 1), 1.0)


@pytest.mark.parametrize("C,bands", [(128, 128), (128, 32), (128, 8), (128, 1), (130, 8), (5, 3), (1, 1)])
def test_band_matrix(C, bands):
    W = smear.BandMatrix(C, bands)
    assert W.shape == (C, C) and W.dtype == np.float64 and (W >= 0).all() and np.allclose(W.sum(axis=1), 1.0, rtol=0, atol=2.0 ** -52)
    groups = np.array_split(np.arange(C), bands)
    assert len(groups) == bands
    want = np.zeros((C, C))
    for g in groups:
        want[np.ix_(g, g)] = 1.0 / len(g)                                          # constant blocks on the diagonal
    assert np.array_equal(W, want)
    if bands == C:
        assert np.array_equal(W, np.eye(C))


@pytest.mark.parametrize("C,bands", [(128, 0), (128, 129), (128, -1), (0, 0)])
def test_band_matrix_refuses(C, bands):
    with pytest.raises(ValueError):
        smear.BandMatrix(C, bands)


# ---- EvaluateSmearSweep against a stub context -------------------------------------------------------------------------------------------
RADIUS, STEP, R = 5, 160, 11


class StubContext:
    """Stands in for the device: labels window j of level l of file b as (j + l + b) % 2 == 0 and counts like the tally."""

    def __init__(self):
        self.calls = []

    def cnn_create(self, tensors, rows, channels):
        return 1

    def eval_smear_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, mix, env_levels,
                         scores, labels, mem_space):
        K = len(mix)
        lengths = np.diff(offsets)
        self.calls.append(dict(B=B, lengths=lengths.tolist(), dtype=wave_dtype, Cn=Cn, hop=hop, mix=np.array(mix), step=step, lpf=lpf,
                               cutoff=cutoff, coefs=np.array(coefs)))
        assert handle == 1 and env_levels is None and mem_space == _lib.MEM_HOST and wave.shape[0] == offsets[-1]
        assert np.asarray(mix).shape == (K, Cn, Cn)
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


def test_evaluate_smear_sweep_groups_and_writes(workdir, capsys):
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    lengths = [2000 + 7 * i for i in range(18)]
    files = write_wavs(workdir, lengths) + write_wavs(workdir, [2500], rate=8000)
    stub = StubContext()
    res = Evaluating.EvaluateSmearSweep(files, spreads=[0.5, 2], bands=[16], hop=160, LPF=True, CUTOFF=40, model=F2CNNModel.glorot(7), ctx=stub)
    # one rate per pass, 16 files at the most
    assert [c["B"] for c in stub.calls] == [16, 2, 1]
    assert stub.calls[0]["lengths"] == lengths[:16] and stub.calls[1]["lengths"] == lengths[16:] and stub.calls[2]["lengths"] == [2500]
    assert [c["step"] for c in stub.calls] == [160, 160, 80] and all(c["hop"] == 160 and c["lpf"] is True and c["cutoff"] == 40 for c in stub.calls)
    # the levels: the spreads first, then the bands; the matrices are those of the group's own centre frequencies
    for c, rate in zip(stub.calls, (16000, 16000, 8000)):
        freqs = filters.centre_freqs(rate, 128, 100)
        assert np.array_equal(c["coefs"], filters.make_erb_filters(rate, freqs))
        assert np.array_equal(c["mix"], np.stack([smear.SmearMatrix(freqs, 0.5), smear.SmearMatrix(freqs, 2.0), smear.BandMatrix(128, 16)]))
    assert not np.array_equal(stub.calls[0]["mix"][0], stub.calls[2]["mix"][0])
    assert list(res) == files
    K = 3
    names = ("0.5ERB", "2ERB", "16bands", "sharp")
    expected = ""
    for i, file in enumerate(files):
        out = os.path.splitext(file)[0] + ".smearsweep.npz"
        archive = np.load(out)
        assert list(archive.files) == list(res[file]) == ["spread_erb", "bands", "windows", "rising", "agree", "agreement", "hop", "timepoints",
                                                          "scores", "labels_0", "labels_1", "labels_2", "labels_sharp"]
        n = _lib.strided_window_count(lengths[i], RADIUS, STEP, 160) if i < 18 else _lib.strided_window_count(2500, RADIUS, 80, 160)
        expected += "File:\t\t{}\n".format(file)
        for l, name in enumerate(names):
            rising = ((np.arange(n) + l + (i % 16 if i < 18 else 0)) % 2 == 0).sum()
            expected += "\tsmear {:>8}\t{} windows\t{} rising\tagreement with sharp {:.4f}\n".format(name, n, rising, (0.0, 1.0, 0.0, 1.0)[l])
        expected += "\t\t{}\tdone ! -> {}\n".format(file, out)
        if i >= 18:
            continue
        saved = dict(archive)
        b = i % 16
        assert saved["windows"].tolist() == [n] * (K + 1) and int(saved["hop"]) == 160
        assert np.array_equal(saved["spread_erb"], [0.5, 2.0, np.nan], equal_nan=True) and saved["spread_erb"].dtype == np.float64
        assert saved["bands"].tolist() == [0, 0, 16] and saved["bands"].dtype == np.int64
        assert saved["scores"].shape == (K + 1, n, 2) and saved["scores"].dtype == np.float32
        assert np.array_equal(saved["timepoints"], RADIUS * STEP + 160 * np.arange(n))
        for l, key in enumerate(("labels_0", "labels_1", "labels_2", "labels_sharp")):
            assert np.array_equal(saved[key], (np.arange(n) + l + b) % 2 == 0), (i, key)
            assert saved["rising"][l] == saved[key].sum() and saved["agree"][l] == (saved[key] == saved["labels_sharp"]).sum()
            assert np.array_equal(saved["scores"][l][:, 1], np.float32(0.25) + np.float32(0.5) * saved[key])
            assert np.array_equal(res[file][key], saved[key])
        assert saved["agreement"].tolist() == [0.0, 1.0, 0.0, 1.0]
    printed = capsys.readouterr().out
    assert printed == expected


def test_the_low_pass_is_off_by_default(workdir):
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    stub = StubContext()
    Evaluating.EvaluateSmearSweep(write_wavs(workdir, [2100]), bands=[8], model=F2CNNModel.glorot(7), ctx=stub)
    call, = stub.calls
    assert call["lpf"] is False and call["cutoff"] == 0.0 and call["hop"] == 1 and call["mix"].shape == (1, 128, 128)


@pytest.mark.parametrize("kw", [dict(), dict(spreads=[0]), dict(spreads=[1, float("nan")]), dict(spreads=[-2]), dict(bands=[0]), dict(bands=[129]),
                                dict(bands=[1.5]), dict(spreads=[1.0] * 60, bands=[8] * 5)])
def test_bad_levels_are_refused_before_anything_is_read(workdir, kw):
    from f2cnn_amd.scripts.CNN import Evaluating
    with pytest.raises(ValueError):
        Evaluating.EvaluateSmearSweep(["does-not-exist.WAV"], ctx=StubContext(), **kw)
