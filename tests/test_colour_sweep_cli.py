"""`cnn noisesweep --colours`: the parts that need no GPU - the command line takes the two options on noisesweep alone and hands
them down, the level grid is colour-major with names like `pink 10dB`, the other commands and the sweep without the option are as
they were; the two C entry points are declared and bound and the binding's constants are the kernel's; and EvaluateNoiseSweep with
colours groups its files and writes its .coloursweep.npz and WAVs, held against a stub context that stands in for the device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, cli, noise


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_parser_takes_the_options():
    args = cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "20,10,0", "--colours",
                                          "white,pink,speech,like:babble.wav,fir:taps.npy", "--noise-taps", "513", "--seed", "4",
                                          "--hop", "frame", "--lpf", "50", "--accuracy", "--resample", "--save-wavs"])
    assert args.colours == ["white", "pink", "speech", "like:babble.wav", "fir:taps.npy"] and args.noise_taps == 513
    assert args.snrs == [20.0, 10.0, 0.0] and args.seed == 4 and args.save_wavs and args.CUTOFF == 50
    assert cli.build_parser().parse_args(["cnn", "noisesweep", "-f", "a.WAV", "--snrs", "3", "--colours", "brown"]).colours == ["brown"]
    assert cli.NOISE_COLOURS == noise.COLOURS
    for word in ("--colours", "--noise-taps", "coloursweep.npz", "pink 10dB", "like:", "fir:"):
        assert word in cli.__doc__, word


@pytest.mark.parametrize("flag,bad", [("--colours", "pink,purple"), ("--colours", ""), ("--colours", "pink,,white"), ("--colours", "like:"),
                                      ("--colours", "fir:"), ("--colours", "wav:a.wav"), ("--noise-taps", "x"), ("--noise-taps", "0"),
                                      ("--noise-taps", "1024"), ("--noise-taps", "-5")])
def test_parser_refuses_malformed_values(flag, bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3", flag + "=" + bad])
    assert e.value.code == 2
    assert flag in capsys.readouterr().err


@pytest.fixture
def no_evaluation(monkeypatch):
    """any evaluation the command line would start is recorded, not run"""
    from f2cnn_amd.scripts.CNN import Evaluating
    seen = []
    for name in ("EvaluateReverbSweep", "EvaluateCutoffSweep", "EvaluateSmearSweep", "EvaluateNoiseSweep", "EvaluateOneWavFile",
                 "EvaluateWithNoise", "EvaluateRandom"):
        monkeypatch.setattr(Evaluating, name, lambda *a, _name=name, **kw: seen.append((_name, a, kw)))
    return seen


def test_sweep_hands_its_options_down(no_evaluation):
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "20,0", "--colours", "pink,like:b.wav", "--seed", "3"]) == 0
    (name, a, kw), = no_evaluation
    assert name == "EvaluateNoiseSweep" and a == (["a.WAV"], [20.0, 0.0])
    assert kw == dict(seed=3, save_wavs=False, colours=["pink", "like:b.wav"])
    del no_evaluation[:]
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "5", "--colours", "speech", "--noise-taps", "257", "--save-wavs"]) == 0
    (name, a, kw), = no_evaluation
    assert kw == dict(seed=0, save_wavs=True, colours=["speech"], noise_taps=257)


def test_without_the_option_every_command_parses_and_calls_as_before(no_evaluation):
    for argv in (["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3"], ["cnn", "eval", "--file", "a.WAV"],
                 ["cnn", "evalnoise", "--file", "a.WAV", "--noise", "3"], ["cnn", "reverbsweep", "--file", "a.WAV", "--t60", "0.2"]):
        args = vars(cli.build_parser().parse_args(argv))
        assert not {"colours", "noise_taps"} & set(args), argv
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3,0"]) == 0
    (name, a, kw), = no_evaluation
    assert name == "EvaluateNoiseSweep" and a == (["a.WAV"], [3.0, 0.0]) and kw == dict(seed=0, save_wavs=False)


@pytest.mark.parametrize("command,rest", [("eval", []), ("evalnoise", ["--noise", "3"]), ("evalrand", []), ("train", []), ("test", []),
                                          ("lpfsweep", ["--cutoffs", "5"]), ("reverbsweep", ["--t60", "0.2"]),
                                          ("smearsweep", ["--spreads", "1"])])
@pytest.mark.parametrize("option", [["--colours", "pink"], ["--noise-taps", "65"]])
def test_the_other_commands_refuse_the_options(no_evaluation, capsys, command, rest, option):
    assert cli.main(["cnn", command, "--file", "a.WAV"] + rest + option) == 1
    out = capsys.readouterr().out
    assert option[0] in out and "noisesweep" in out and no_evaluation == []
    if command in cli.SWEEPS:
        assert "is not supported by " + command in out


def test_colours_need_levels_and_taps_need_colours(no_evaluation, capsys):
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--colours", "pink"]) == 1
    assert capsys.readouterr().out.startswith("Please use --snrs")                # like a sweep without levels
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3", "--noise-taps", "65"]) == 1
    assert "--noise-taps belongs to --colours" in capsys.readouterr().out
    assert no_evaluation == []


def test_at_most_64_levels(no_evaluation, capsys):
    snrs = ",".join(str(v) for v in range(13))
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", snrs, "--colours", "white,pink,brown,speech,fir:a.npy"]) == 1
    out = capsys.readouterr().out
    assert "at most 64 levels" in out and "5 colours x 13 SNRs = 65" in out and no_evaluation == []
    snrs = ",".join(str(v) for v in range(16))
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", snrs, "--colours", "white,pink,brown,speech"]) == 0
    assert len(no_evaluation) == 1


def test_the_level_grid_is_colour_major():
    from f2cnn_amd.scripts.CNN import Evaluating
    grid = Evaluating.ColourLevels(["pink", "like:/x/babble.wav", "fir:t.npy"], [10.0, -3.5])
    assert grid == [("pink", "pink", 10.0), ("pink", "pink", -3.5), ("like:/x/babble.wav", "babble", 10.0),
                    ("like:/x/babble.wav", "babble", -3.5), ("fir:t.npy", "t", 10.0), ("fir:t.npy", "t", -3.5)]
    assert Evaluating.ColourLevels("white,speech", [0.0]) == [("white", "white", 0.0), ("speech", "speech", 0.0)]
    assert len(Evaluating.ColourLevels(["pink"] * 8, range(8))) == 64
    for colours, snrs in (([], [3.0]), (["purple"], [3.0]), (["pink", ""], [3.0]), (["like:"], [3.0]), (["pink"] * 5, range(13))):
        with pytest.raises(ValueError):
            Evaluating.ColourLevels(colours, snrs)


# ---- the C entry points -----------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+f2_shaped_noise_levels\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_shaped_noise_levels is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["f2_ctx* ctx", "const void* wave", "int wave_dtype", "const int64_t* offsets", "int B", "const double* snr_db",
                      "const double* fir", "const int64_t* fir_offsets", "int K", "uint64_t seed", "double* noisy", "double* sigma_or_null",
                      "int mem_space"]
    res, args = _lib.SIGNATURES["f2_shaped_noise_levels"]
    assert res is ctypes.c_int and len(args) == len(params) and args[9] is ctypes.c_uint64
    m = re.search(r"\bint\s+f2_eval_shaped_noise_sweep\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_eval_shaped_noise_sweep is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    white = re.search(r"\bint\s+f2_eval_noise_sweep\s*\(([^;]*)\)\s*;", code)
    white = [" ".join(p.split()) for p in white.group(1).split(",")]
    # the white sweep's parameters with the taps and their offsets behind snr_db
    assert params == white[:15] + ["const double* fir", "const int64_t* fir_offsets"] + white[15:]
    res, args = _lib.SIGNATURES["f2_eval_shaped_noise_sweep"]
    base = _lib.SIGNATURES["f2_eval_noise_sweep"][1]
    assert res is ctypes.c_int and args == base[:15] + [ctypes.c_void_p] * 2 + base[15:]
    for word in ("acc = fma(h[t], z[i-t], acc)", "(low, 0xffffffff, l, b)", "mod 2^64", "sum h^2 = 1", "fma(1.0, z, 0.0) is z",
                 "F2_SHAPED_MAX_TAPS", "f2_version stays 114"):
        assert word in text, word
    for name in ("shaped_noise_levels", "eval_shaped_noise_sweep"):
        assert {"snr_db", "firs", "seed"} <= set(inspect.signature(getattr(_lib.Context, name)).parameters)
    from f2cnn_amd.scripts.CNN import Evaluating
    p = inspect.signature(Evaluating.EvaluateNoiseSweep).parameters
    assert list(p)[-2:] == ["colours", "noise_taps"] and p["colours"].default is None and p["noise_taps"].default == 1025


def test_the_bindings_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "f2cnn_amd", "csrc", "f2_internal.h")).read()
    define = lambda name: int(re.search(r"^#define\s+" + name + r"\s+(\d+)\s*$", text, flags=re.M).group(1))
    assert _lib.SHAPED_BLOCK == define("F2_SHAPED_BLOCK") == 1024
    assert _lib.SHAPED_MAX_TAPS == define("F2_SHAPED_MAX_TAPS") == noise.MAX_TAPS == 2048
    assert _lib.SHAPED_MAX_LEVELS == define("F2_SHAPED_MAX_LEVELS") == 64
    from f2cnn_amd.scripts.CNN import Evaluating
    assert Evaluating.COLOUR_LEVELS_MAX == cli.NOISE_LEVELS_MAX == 64


def test_pack_firs_wants_one_filter_per_level():
    taps, fo = _lib._pack_firs([np.ones(1), [0.6, 0.8]], 2)
    assert taps.tolist() == [1.0, 0.6, 0.8] and fo.tolist() == [0, 1, 3] and taps.dtype == np.float64 and fo.dtype == np.int64
    with pytest.raises(ValueError, match="one per level"):
        _lib._pack_firs([np.ones(1)], 2)


# ---- EvaluateNoiseSweep(colours=...) against a stub context -----------------------------------------------------------------
RADIUS = 5


class StubContext:
    """Stands in for the device: labels window j of level l of file b as (j + l + b) % 2 == 0, counts like the tally, says
    sigma = l + 1 + b / 16 for level l of file b (0 for the clean level) and, asked for the noisy waveforms, returns level l as the
    clean samples times l + 1. It has no white sweep: a call of it would be an AttributeError."""

    def __init__(self):
        self.calls = []

    def cnn_create(self, tensors, rows, channels):
        return 1

    def eval_shaped_noise_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, snr_db,
                                firs, seed, noisy, scores, labels, mem_space):
        K = len(snr_db)
        lengths = np.diff(offsets)
        self.calls.append(dict(B=B, lengths=lengths.tolist(), step=step, hop=hop, lpf=lpf, cutoff=cutoff, snr=list(snr_db), seed=seed,
                               firs=[np.array(h) for h in firs], noisy=noisy is not None))
        assert handle == 1 and scores is None and mem_space == _lib.MEM_HOST and wave.shape[0] == offsets[-1] and len(firs) == K
        per = [_lib.strided_window_count(int(n), radius, step, hop) for n in lengths] * (K + 1)
        wo = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        assert labels.shape == (wo[-1],)
        for u in range((K + 1) * B):
            l, b = divmod(u, B)
            labels[wo[u]:wo[u + 1]] = (np.arange(per[u]) + l + b) % 2 == 0
        if noisy is not None:
            for l in range(K + 1):
                noisy[l * offsets[-1]:(l + 1) * offsets[-1]] = wave.astype(np.float64) * (l + 1)
        sigma = np.array([(l + 1 + b / 16.0) if l < K else 0.0 for l in range(K + 1) for b in range(B)])
        stats = np.zeros(((K + 1) * B, 2), np.int64)
        for u in range((K + 1) * B):
            mine, ref = labels[wo[u]:wo[u + 1]], labels[wo[K * B + u % B]:wo[K * B + u % B + 1]]
            stats[u] = mine.sum(), (mine == ref).sum()
        return wo, sigma, stats


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    from f2cnn_amd import config
    monkeypatch.chdir(tmp_path)
    config.write_default()
    return tmp_path


def write_wavs(workdir, lengths, rate=16000):
    from scipy.io import wavfile
    files = []
    rng = np.random.default_rng(3)
    for i, n in enumerate(lengths):
        path = str(workdir / "F{}_{}.WAV".format(rate, i))
        wavfile.write(path, rate, (rng.standard_normal(n) * 3000).astype(np.int16))
        files.append(path)
    return files


def test_evaluate_colour_sweep_groups_names_and_writes(workdir, capsys):
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    lengths = [2000 + 7 * i for i in range(17)]
    files = write_wavs(workdir, lengths) + write_wavs(workdir, [2500], rate=8000)
    np.save("mine.npy", np.array([3.0, 4.0]))
    stub = StubContext()
    res = Evaluating.EvaluateNoiseSweep(files, [10, -3.5], seed=7, hop=160, model=F2CNNModel.glorot(7), ctx=stub,
                                        colours=["white", "pink", "fir:mine.npy"], noise_taps=65)
    K = 6
    assert [c["B"] for c in stub.calls] == [16, 1, 1] and [c["step"] for c in stub.calls] == [160, 160, 80]
    for c, rate in zip(stub.calls, (16000, 16000, 8000)):
        assert c["snr"] == [10.0, -3.5] * 3 and c["seed"] == 7 and c["hop"] == 160 and not c["lpf"] and not c["noisy"]
        assert [len(h) for h in c["firs"]] == [1, 1, 65, 65, 2, 2]
        assert np.array_equal(c["firs"][2], noise.ColourFIR("pink", rate, 65)) and c["firs"][4].tolist() == [0.6, 0.8]
    names = ["white 10dB", "white -3.5dB", "pink 10dB", "pink -3.5dB", "mine 10dB", "mine -3.5dB", "clean"]
    expected = ""
    for i, file in enumerate(files):
        stem = os.path.basename(os.path.splitext(file)[0])
        out = os.path.join("OutputWavFiles", "addedNoise", stem + ".coloursweep.npz")
        archive = np.load(out)
        assert list(archive.files) == list(res[file]) == ["snr_db", "colours", "sigma", "windows", "rising", "agree", "agreement", "seed",
                                                          "hop"] + ["labels_%d" % k for k in range(K)] + ["labels_clean", "fir",
                                                                                                          "fir_offsets"]
        saved = dict(archive)
        rate, n_samples = (16000, lengths[i]) if i < 17 else (8000, 2500)
        n = _lib.strided_window_count(n_samples, RADIUS, rate // 100, 160)
        b = i % 16 if i < 17 else 0
        assert saved["windows"].tolist() == [n] * (K + 1) and int(saved["hop"]) == 160 and int(saved["seed"]) == 7
        assert saved["snr_db"].tolist() == [10.0, -3.5] * 3 and saved["sigma"].tolist() == [l + 1 + b / 16.0 for l in range(K)] + [0.0]
        assert saved["colours"].tolist() == ["white", "white", "pink", "pink", "mine", "mine"]
        assert saved["fir_offsets"].tolist() == [0, 1, 2, 67, 132, 134, 136] and saved["fir_offsets"].dtype == np.int64
        assert np.array_equal(saved["fir"][2:67], noise.ColourFIR("pink", rate, 65)) and saved["fir"][132:134].tolist() == [0.6, 0.8]
        clean = (np.arange(n) + K + b) % 2 == 0
        expected += "File:\t\t{}\n".format(file)
        for l, name in enumerate(names):
            mine = (np.arange(n) + l + b) % 2 == 0
            key = "labels_clean" if l == K else "labels_%d" % l
            assert np.array_equal(saved[key], mine) and saved["rising"][l] == mine.sum() and saved["agree"][l] == (mine == clean).sum()
            expected += "\t{:>16}\t{} windows\t{} rising\tagreement with clean {:.4f}\n".format(name, n, mine.sum(), (mine == clean).sum() / n)
        expected += "\t\t{}\tdone ! -> {}\n".format(file, out)
    assert capsys.readouterr().out == expected
    assert sorted(os.listdir(os.path.join("OutputWavFiles", "addedNoise"))) == sorted(
        os.path.basename(os.path.splitext(f)[0]) + ".coloursweep.npz" for f in files)       # no .sweep.npz, no WAV


def test_saved_wavs_are_named_by_colour_and_level(workdir):
    from scipy.io import wavfile
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    file, = write_wavs(workdir, [2600])
    open(os.path.splitext(file)[0] + ".PHN", "w").write("0 10 x\n")
    stub = StubContext()
    Evaluating.EvaluateNoiseSweep(file, [20, 2.5], LPF=True, CUTOFF=40, save_wavs=True, model=F2CNNModel.glorot(7), ctx=stub,
                                  colours="speech,brown")
    call, = stub.calls
    assert call["lpf"] and call["cutoff"] == 40 and call["noisy"] and call["hop"] == 1 and [len(h) for h in call["firs"]] == [1025] * 4
    stem = os.path.basename(os.path.splitext(file)[0])
    clean = wavfile.read(file)[1].astype(np.float64)
    names = ["_speech_20dB", "_speech_2.5dB", "_brown_20dB", "_brown_2.5dB"]
    for l, name in enumerate(names):
        target = os.path.join("OutputWavFiles", "addedNoise", stem + name)
        rate, data = wavfile.read(target + ".WAV")
        assert rate == 16000 and np.array_equal(data, clean * (l + 1))
        assert os.path.exists(target + ".PHN") and not os.path.exists(target + ".FB")
    assert sorted(os.listdir(os.path.join("OutputWavFiles", "addedNoise"))) == sorted(
        [stem + ".coloursweep.npz"] + [stem + name + ext for name in names for ext in (".WAV", ".PHN")])


@pytest.mark.parametrize("kw", [dict(colours=[]), dict(colours=["purple"]), dict(colours=["pink"], noise_taps=64),
                                dict(colours=["pink"], noise_taps=2049), dict(colours=["pink"] * 33), dict(colours=["like:"])])
def test_bad_colours_are_refused_before_anything_is_read(kw):
    from f2cnn_amd.scripts.CNN import Evaluating
    with pytest.raises(ValueError):
        Evaluating.EvaluateNoiseSweep(["does-not-exist.WAV"], [3.0, 0.0], ctx=StubContext(), **kw)
