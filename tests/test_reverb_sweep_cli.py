"""`cnn reverbsweep`: the parts that need no GPU - the command line takes the new command and its flags, refuses what the sweep
does not do and leaves the other commands as they were; the two C entry points are declared and bound and the tile constants of
the binding are those of the kernel; SyntheticRIR and LoadRIR build what their docstrings say; and EvaluateReverbSweep groups its
files and writes its .npz, held against a stub context that stands in for the device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, cli, reverb


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_parser_takes_the_sweep():
    args = cli.build_parser().parse_args(["cnn", "reverbsweep", "--file", "a.WAV", "--t60", "0.2,0.4,0.8", "--hop", "frame", "--drr", "-3",
                                          "--rir", "room.wav,hall.wav", "--seed", "4", "--save-wavs", "--lpf", "50"])
    assert args.cnn_command == "reverbsweep" and args.file == "a.WAV" and args.hop == "frame"
    assert args.t60 == [0.2, 0.4, 0.8] and args.rir == ["room.wav", "hall.wav"] and args.drr == -3.0 and args.seed == 4
    assert args.save_wavs and args.CUTOFF == 50
    assert cli.build_parser().parse_args(["cnn", "reverbsweep", "-f", "a.WAV", "--t60", "1.6"]).t60 == [1.6]
    assert "reverbsweep" in cli.CNN and "reverbsweep" in cli.__doc__ and "--t60" in cli.__doc__ and "--rir" in cli.__doc__


@pytest.mark.parametrize("bad", ["0.2,x", "", "0.2,,0.4", "nan", "inf,3", "0", "-0.5", "0.4,0"])
def test_parser_refuses_a_malformed_list(bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "reverbsweep", "--file", "a.WAV", "--t60=" + bad])
    assert e.value.code == 2
    assert "--t60" in capsys.readouterr().err


@pytest.mark.parametrize("flag,bad", [("--rir", "a.wav,,b.wav"), ("--rir", ""), ("--drr", "x"), ("--drr", "nan")])
def test_parser_refuses_malformed_rir_and_drr(flag, bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "reverbsweep", "--file", "a.WAV", "--t60", "0.2", flag + "=" + bad])
    assert e.value.code == 2
    assert flag in capsys.readouterr().err


@pytest.fixture
def no_evaluation(monkeypatch):
    """any evaluation the command line would start is recorded, not run"""
    from f2cnn_amd.scripts.CNN import Evaluating
    seen = []
    for name in ("EvaluateReverbSweep", "EvaluateCutoffSweep", "EvaluateNoiseSweep", "EvaluateOneWavFile", "EvaluateWithNoise",
                 "EvaluateRandom"):
        monkeypatch.setattr(Evaluating, name, lambda *a, _name=name, **kw: seen.append((_name, a, kw)))
    return seen


@pytest.mark.parametrize("extra,word", [(["--figure"], "--figure"), (["--occlusion"], "--occlusion"), (["--occlusion", "8:4"], "--occlusion")])
def test_sweep_refuses_figure_and_occlusion(no_evaluation, capsys, extra, word):
    assert cli.main(["cnn", "reverbsweep", "--file", "a.WAV", "--t60", "0.2,0.4"] + extra) == 1
    out = capsys.readouterr().out
    assert word in out and "reverbsweep" in out and "eval" in out and no_evaluation == []


def test_sweep_needs_a_file_and_a_room(no_evaluation, capsys):
    assert cli.main(["cnn", "reverbsweep", "--t60", "0.2"]) == 1
    assert capsys.readouterr().out == "Please use --file or -f to give input file\n"
    assert cli.main(["cnn", "reverbsweep", "--file", "a.WAV"]) == 1
    out = capsys.readouterr().out
    assert out.startswith("Please use --t60") and "--rir" in out
    assert no_evaluation == []


def test_sweep_hands_its_options_down(no_evaluation, monkeypatch, tmp_path):
    from f2cnn_amd import config
    monkeypatch.chdir(tmp_path)
    config.write_default()
    assert cli.main(["cnn", "reverbsweep", "--file", "a.WAV", "--t60", "0.2,0.8", "--hop", "frame", "--accuracy", "--resample", "--model",
                     "m.npz", "--lpf", "50"]) == 0
    (name, a, kw), = no_evaluation
    assert name == "EvaluateReverbSweep" and a == (["a.WAV"],)
    assert kw == dict(t60s=[0.2, 0.8], rirs=(), drr_db=0.0, seed=0, save_wavs=False, hop=config.F2Config().step, accuracy="reference",
                      resample=True, model="m.npz", LPF=True, CUTOFF=50)
    del no_evaluation[:]
    assert cli.main(["cnn", "reverbsweep", "--file", "a.WAV", "--rir", "room.wav", "--drr", "6", "--seed", "3", "--save-wavs"]) == 0
    (name, a, kw), = no_evaluation
    assert kw == dict(t60s=(), rirs=["room.wav"], drr_db=6.0, seed=3, save_wavs=True)


def test_other_commands_parse_as_before(no_evaluation):
    for argv in (["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3"], ["cnn", "eval", "--file", "a.WAV"],
                 ["cnn", "lpfsweep", "--file", "a.WAV", "--cutoffs", "5"]):
        args = vars(cli.build_parser().parse_args(argv))
        assert not {"t60", "rir", "drr"} & set(args), argv
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3,0"]) == 0
    (name, a, kw), = no_evaluation
    assert name == "EvaluateNoiseSweep" and a == (["a.WAV"], [3.0, 0.0]) and kw == dict(seed=0, save_wavs=False)


# ---- the C entry points -----------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+f2_reverb_levels\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_reverb_levels is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["f2_ctx* ctx", "const void* wave", "int wave_dtype", "const int64_t* offsets", "int B", "const double* rir",
                      "const int64_t* rir_offsets", "int K", "double* levels", "int mem_space"]
    res, args = _lib.SIGNATURES["f2_reverb_levels"]
    assert res is ctypes.c_int and len(args) == len(params)
    m = re.search(r"\bint\s+f2_eval_reverb_sweep\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_eval_reverb_sweep is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["f2_ctx* ctx", "const f2_cnn* cnn", "const void* wave", "int wave_dtype", "const int64_t* offsets",
                      "const double* coefs", "int B", "int C", "int lpf", "double cutoff_hz", "int fft_precision", "int radius", "int step",
                      "int hop", "const double* rir", "const int64_t* rir_offsets", "int K", "double* wet_or_null", "float* scores_or_null",
                      "uint8_t* labels_or_null", "int64_t* window_offsets_or_null", "int64_t* stats_or_null", "int mem_space"]
    res, args = _lib.SIGNATURES["f2_eval_reverb_sweep"]
    assert res is ctypes.c_int and len(args) == len(params)
    # the binding is f2_eval_batch_strided's up to hop, then the responses, then the outputs
    base = _lib.SIGNATURES["f2_eval_batch_strided"][1]
    assert args[:14] == base[:14] and args[14:17] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert args[17:] == [ctypes.c_void_p] * 5 + [ctypes.c_int]
    for word in ("acc = fma(h[t], x[k-t], acc)", "numpy.convolve(x, h)[:n]", "ascending t", "F2_REVERB_MAX_TAPS"):
        assert word in text, word
    assert "rirs" in inspect.signature(_lib.Context.eval_reverb_sweep).parameters
    assert "rirs" in inspect.signature(_lib.Context.reverb_levels).parameters
    from f2cnn_amd.scripts.CNN import Evaluating
    p = inspect.signature(Evaluating.EvaluateReverbSweep).parameters
    assert list(p) == ["files", "t60s", "rirs", "drr_db", "seed", "hop", "LPF", "CUTOFF", "model", "save_wavs", "ctx", "accuracy",
                       "resample"]
    assert [p[k].default for k in list(p)[1:]] == [(), (), 0.0, 0, None, False, 50, "last_trained_model", False, None, None, False]


def test_the_bindings_tile_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "f2cnn_amd", "csrc", "f2_internal.h")).read()
    define = lambda name: int(re.search(r"^#define\s+" + name + r"\s+(\d+)\s*$", text, flags=re.M).group(1))
    assert _lib.REVERB_BLOCK == define("F2_REVERB_BLOCK")
    assert _lib.REVERB_TAP_CHUNK == define("F2_REVERB_TAP_CHUNK")
    assert _lib.REVERB_MAX_TAPS == define("F2_REVERB_MAX_TAPS") == reverb.MAX_TAPS == 32768
    assert define("F2_REVERB_MAX_LEVELS") == 64


def test_pack_rirs():
    taps, ro = _lib._pack_rirs([np.array([1.0, 0.5]), [2], np.arange(3, dtype=np.float32)])
    assert taps.dtype == np.float64 and taps.tolist() == [1.0, 0.5, 2.0, 0.0, 1.0, 2.0] and ro.tolist() == [0, 2, 3, 6]
    taps, ro = _lib._pack_rirs([])
    assert len(taps) == 0 and ro.tolist() == [0] and ro.dtype == np.int64


# ---- SyntheticRIR / LoadRIR -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t60,framerate,drr", [(0.1, 16000, 0.0), (0.4, 16000, 6.0), (0.25, 8000, -3.0), (0.30001, 16000, 0.0)])
def test_synthetic_rir_is_the_polack_model(t60, framerate, drr):
    h = reverb.SyntheticRIR(t60, framerate, drr_db=drr, seed=9, level=2)
    L = max(1, int(np.ceil(t60 * framerate)))
    assert h.dtype == np.float64 and h.shape == (L,) and h[0] == 1.0 and np.isfinite(h).all()
    assert abs(np.dot(h[1:], h[1:]) / 10 ** (-drr / 10) - 1) <= 1e-12
    # the envelope: the noise it multiplies is the documented stream, so dividing it out leaves g * 10^(-3 k / (t60 framerate))
    w = np.random.default_rng([9, 2]).standard_normal(L)
    env = h[1:] / w[1:]
    assert (env > 0).all()
    ratio = env[-1] / env[0]                                  # taps 1 and L - 1: 60 dB apart but for the two end taps
    assert 1e-3 <= ratio <= 1e-3 * 10 ** (3 / L * 3), ratio
    k = np.arange(1, L)
    assert np.allclose(env / env[0], 10.0 ** (-3.0 * (k - 1) / (t60 * framerate)), rtol=1e-12)


def test_synthetic_rir_streams():
    a = reverb.SyntheticRIR(0.2, 16000, seed=1, level=0)
    assert np.array_equal(a.view(np.uint8), reverb.SyntheticRIR(0.2, 16000, seed=1, level=0).view(np.uint8))
    assert not np.array_equal(a, reverb.SyntheticRIR(0.2, 16000, seed=1, level=1))
    assert not np.array_equal(a, reverb.SyntheticRIR(0.2, 16000, seed=2, level=0))
    assert reverb.SyntheticRIR(1e-6, 16000).tolist() == [1.0]                      # one tap: the direct path alone
    assert len(reverb.SyntheticRIR(32768 / 16000.0, 16000)) == 32768               # the longest response


@pytest.mark.parametrize("t60", [0, -1.0, float("nan"), float("inf"), 2.1, 1e300])
def test_synthetic_rir_refusals(t60):
    with pytest.raises(ValueError, match="32768" if t60 in (2.1, 1e300) else "t60"):
        reverb.SyntheticRIR(t60, 16000)


def test_load_rir(tmp_path):
    from scipy.io import wavfile
    h = np.zeros(400, np.int16)
    h[37], h[38], h[120], h[10] = -20000, 5000, -2500, 300                       # something before the peak, a negative peak
    path = str(tmp_path / "room.wav")
    wavfile.write(path, 16000, h)
    got = reverb.LoadRIR(path, 16000)
    assert got.dtype == np.float64 and got.shape == (400 - 37,) and got[0] == 1.0
    assert got[1] == -0.25 and got[120 - 37] == 0.125 and np.abs(got).max() == 1.0
    with pytest.raises(ValueError, match="8000"):
        reverb.LoadRIR(path, 8000)
    stereo = str(tmp_path / "stereo.wav")
    wavfile.write(stereo, 16000, np.stack([h, h], axis=1))
    with pytest.raises(ValueError, match="stereo.wav"):
        reverb.LoadRIR(stereo, 16000)
    silent = str(tmp_path / "silent.wav")
    wavfile.write(silent, 16000, np.zeros(10, np.int16))
    with pytest.raises(ValueError, match="silent.wav"):
        reverb.LoadRIR(silent, 16000)
    long = str(tmp_path / "long.wav")
    wavfile.write(long, 16000, np.concatenate([[30000], np.ones(32768)]).astype(np.int16))
    with pytest.raises(ValueError, match="32768"):
        reverb.LoadRIR(long, 16000)
    flt = str(tmp_path / "float.wav")
    wavfile.write(flt, 16000, np.array([0.0, 0.5, -0.25], np.float32))
    assert reverb.LoadRIR(flt, 16000).tolist() == [1.0, -0.5]


# ---- EvaluateReverbSweep against a stub context -----------------------------------------------------------------------------
RADIUS, STEP, R = 5, 160, 11


class StubContext:
    """Stands in for the device: labels window j of level l of file b as (j + l + b) % 2 == 0, counts like the tally and, asked
    for the wet waveforms, returns level l as the dry samples times l + 1."""

    def __init__(self):
        self.calls = []

    def cnn_create(self, tensors, rows, channels):
        return 1

    def eval_reverb_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, rirs, wet,
                          scores, labels, mem_space):
        K = len(rirs)
        lengths = np.diff(offsets)
        self.calls.append(dict(B=B, lengths=lengths.tolist(), dtype=wave_dtype, Cn=Cn, hop=hop, step=step, lpf=lpf, cutoff=cutoff,
                               rirs=[np.array(h) for h in rirs], wet=wet is not None))
        assert handle == 1 and scores is None and mem_space == _lib.MEM_HOST and wave.shape[0] == offsets[-1]
        per = [_lib.strided_window_count(int(n), radius, step, hop) for n in lengths] * (K + 1)
        wo = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        assert labels.shape == (wo[-1],)
        for u in range((K + 1) * B):
            l, b = divmod(u, B)
            labels[wo[u]:wo[u + 1]] = (np.arange(per[u]) + l + b) % 2 == 0
        if wet is not None:
            assert wet.shape == ((K + 1) * offsets[-1],) and wet.dtype == np.float64
            for l in range(K + 1):
                wet[l * offsets[-1]:(l + 1) * offsets[-1]] = wave.astype(np.float64) * (l + 1)
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


def test_evaluate_reverb_sweep_groups_and_writes(workdir, capsys):
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    lengths = [2000 + 7 * i for i in range(18)]
    files = write_wavs(workdir, lengths) + write_wavs(workdir, [2500], rate=8000)
    stub = StubContext()
    res = Evaluating.EvaluateReverbSweep(files, t60s=[0.05, 0.2], drr_db=3.0, seed=5, hop=160, model=F2CNNModel.glorot(7), ctx=stub)
    # one rate per pass, 16 files at the most; the responses of a rate are built once
    assert [c["B"] for c in stub.calls] == [16, 2, 1]
    assert stub.calls[0]["lengths"] == lengths[:16] and stub.calls[1]["lengths"] == lengths[16:] and stub.calls[2]["lengths"] == [2500]
    assert [c["step"] for c in stub.calls] == [160, 160, 80] and all(c["hop"] == 160 and not c["lpf"] and not c["wet"] for c in stub.calls)
    assert [[len(h) for h in c["rirs"]] for c in stub.calls] == [[800, 3200], [800, 3200], [400, 1600]]
    for l in range(2):
        want = reverb.SyntheticRIR((0.05, 0.2)[l], 16000, 3.0, 5, l)
        assert all(np.array_equal(c["rirs"][l], want) for c in stub.calls[:2])
    assert list(res) == files
    K = 2
    expected = ""
    for i, file in enumerate(files):
        stem = os.path.basename(os.path.splitext(file)[0])
        out = os.path.join("OutputWavFiles", "reverb", stem + ".reverbsweep.npz")
        archive = np.load(out)
        assert list(archive.files) == list(res[file]) == ["t60", "rir_files", "drr_db", "seed", "taps", "windows", "rising", "agree",
                                                          "agreement", "hop", "labels_0", "labels_1", "labels_dry", "rir_0", "rir_1"]
        saved = dict(archive)
        rate, n_samples = (16000, lengths[i]) if i < 18 else (8000, 2500)
        n = _lib.strided_window_count(n_samples, RADIUS, rate // 100, 160)
        b = i % 16 if i < 18 else 0
        expected += "File:\t\t{}\n".format(file)
        for l, name in enumerate(("T60 0.05s", "T60 0.2s", "dry")):
            expected += "\t{:>12}\t{} windows\t{} rising\tagreement with dry {:.4f}\n".format(
                name, n, ((np.arange(n) + l + b) % 2 == 0).sum(), (1.0, 0.0, 1.0)[l])
        expected += "\t\t{}\tdone ! -> {}\n".format(file, out)
        assert saved["windows"].tolist() == [n] * (K + 1) and int(saved["hop"]) == 160 and saved["t60"].tolist() == [0.05, 0.2]
        assert float(saved["drr_db"]) == 3.0 and int(saved["seed"]) == 5 and saved["rir_files"].shape == (0,)
        assert saved["taps"].tolist() == [rate // 20, rate // 5]
        for l, key in enumerate(("labels_0", "labels_1", "labels_dry")):
            assert np.array_equal(saved[key], (np.arange(n) + l + b) % 2 == 0), (i, key)
            assert saved["rising"][l] == saved[key].sum() and saved["agree"][l] == (saved[key] == saved["labels_dry"]).sum()
            assert np.array_equal(res[file][key], saved[key])
        for l in range(K):
            assert np.array_equal(saved["rir_%d" % l], reverb.SyntheticRIR((0.05, 0.2)[l], rate, 3.0, 5, l))
        assert saved["agreement"].tolist() == [1.0, 0.0, 1.0]
    printed = capsys.readouterr().out
    assert printed.count("agreement with dry") == 19 * (K + 1) and "T60 0.05s" in printed and "T60 0.2s" in printed
    assert printed.count("File:") == 19 and printed.count("done !") == 19
    assert printed == expected


def test_measured_responses_low_pass_and_saved_wavs(workdir, capsys):
    from scipy.io import wavfile
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    file, = write_wavs(workdir, [2600])
    for ext in (".PHN", ".WRD"):
        open(os.path.splitext(file)[0] + ext, "w").write("0 10 x\n")
    room = str(workdir / "room.wav")
    wavfile.write(room, 16000, np.array([0, 100, 16000, -4000, 2000], np.int16))
    stub = StubContext()
    res = Evaluating.EvaluateReverbSweep(file, t60s=[0.1], rirs=[room], LPF=True, CUTOFF=40, save_wavs=True, model=F2CNNModel.glorot(7),
                                         ctx=stub)[file]
    call, = stub.calls
    assert call["lpf"] and call["cutoff"] == 40 and call["wet"] and call["hop"] == 1
    assert call["rirs"][1].tolist() == [1.0, -0.25, 0.125]                        # levels: the t60s, then the files
    assert res["rir_files"].tolist() == [room] and res["taps"].tolist() == [1600, 3] and res["rir_1"].tolist() == [1.0, -0.25, 0.125]
    stem = os.path.basename(os.path.splitext(file)[0])
    dry = wavfile.read(file)[1].astype(np.float64)
    for l, name in enumerate(("_T60_0.1s", "_room")):
        target = os.path.join("OutputWavFiles", "reverb", stem + name)
        rate, data = wavfile.read(target + ".WAV")
        assert rate == 16000 and np.array_equal(data, dry * (l + 1))
        assert os.path.exists(target + ".PHN") and os.path.exists(target + ".WRD") and not os.path.exists(target + ".FB")
    assert list(res) == ["t60", "rir_files", "drr_db", "seed", "taps", "windows", "rising", "agree", "agreement", "hop", "labels_0",
                         "labels_1", "labels_dry", "rir_0", "rir_1"]
    assert sorted(os.listdir(os.path.join("OutputWavFiles", "reverb"))) == sorted(
        [stem + ".reverbsweep.npz"] + [stem + name + ext for name in ("_T60_0.1s", "_room") for ext in (".WAV", ".PHN", ".WRD")])
    printed = capsys.readouterr().out
    assert "room.wav" in printed and printed.count("agreement with dry") == 3
    n = _lib.strided_window_count(2600, RADIUS, STEP, 1)
    assert printed == "File:\t\t{}\n".format(file) + "".join(
        "\t{:>12}\t{} windows\t{} rising\tagreement with dry {:.4f}\n".format(name, n, n // 2, agreement)
        for name, agreement in (("T60 0.1s", 1.0), ("room.wav", 0.0), ("dry", 1.0))) + \
        "\t\t{}\tdone ! -> {}\n".format(file, os.path.join("OutputWavFiles", "reverb", stem + ".reverbsweep.npz"))


@pytest.mark.parametrize("kw", [dict(), dict(t60s=[0]), dict(t60s=[float("nan")]), dict(t60s=[0.2, -1]), dict(t60s=[0.1] * 65),
                                dict(t60s=[0.2], drr_db=float("inf"))])
def test_bad_lists_are_refused_before_anything_is_read(kw):
    from f2cnn_amd.scripts.CNN import Evaluating
    with pytest.raises(ValueError):
        Evaluating.EvaluateReverbSweep(["does-not-exist.WAV"], ctx=StubContext(), **kw)
