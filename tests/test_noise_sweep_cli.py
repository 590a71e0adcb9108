"""`cnn noisesweep`: the parts that need no GPU - the command line takes the new command and its options and leaves
`cnn evalnoise` as it was, the C entry point is declared, exported and bound, the library says version 109, and
EvaluateNoiseSweep groups its files, prints its lines and writes its .npz and WAVs, held against a stub context that stands in for
the device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, build, cli


def test_parser_takes_the_sweep():
    args = cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "20,10,-3", "--seed", "5", "--hop", "frame"])
    assert args.cnn_command == "noisesweep" and args.file == "a.WAV"
    assert args.snrs == [20.0, 10.0, -3.0] and args.seed == 5 and args.hop == "frame" and args.save_wavs is False
    assert cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "0", "--save-wavs"]).save_wavs is True
    assert "noisesweep" in cli.CNN and "noisesweep" in cli.__doc__


@pytest.mark.parametrize("bad", ["20,x", "", "20,,10", "nan", "inf,3"])
def test_parser_refuses_a_malformed_list(bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", bad])
    assert e.value.code == 2
    assert "--snrs" in capsys.readouterr().err


def test_evalnoise_parses_as_before():
    args = vars(cli.build_parser().parse_args(["cnn", "evalnoise", "--file", "a.WAV", "--noise", "-3"]))
    before = dict(configure=False, file="a.WAV", inputFile=None, labelFile=None, model=None, cnn_command="evalnoise", CUTOFF=None,
                  count=None, SNRdB=-3.0, hop=None)
    assert {k: args[k] for k in before} == before
    assert sorted(set(args) - set(before)) == ["save_wavs", "seed", "snrs"]
    assert args["snrs"] is None and args["seed"] is None and args["save_wavs"] is False


def test_sweep_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+f2_eval_noise_sweep\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_eval_noise_sweep is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert len(params) == 24
    assert params[13:17] == ["int hop", "const double* snr_db", "int K", "uint64_t seed"]
    assert params[17:] == ["double* noisy_or_null", "float* scores_or_null", "uint8_t* labels_or_null", "int64_t* window_offsets_or_null",
                           "double* sigma_or_null", "int64_t* stats_or_null", "int mem_space"]
    for word in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "Evaluating.py:199"):
        assert word in text, word
    res, args = _lib.SIGNATURES["f2_eval_noise_sweep"]
    assert res is ctypes.c_int and len(args) == len(params)
    # the binding is f2_eval_batch_strided's up to `hop`, then the levels and the seed, then the outputs
    base = _lib.SIGNATURES["f2_eval_batch_strided"][1]
    assert args[:14] == base[:14] and args[14:17] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64]
    assert args[17:] == [ctypes.c_void_p] * 6 + [ctypes.c_int]
    p = inspect.signature(_lib.Context.eval_noise_sweep).parameters
    assert "snr_db" in p and "seed" in p and "hop" in p
    from f2cnn_amd.scripts.CNN import Evaluating
    p = inspect.signature(Evaluating.EvaluateNoiseSweep).parameters
    assert list(p)[:2] == ["files", "SNRdBs"]
    assert (p["seed"].default, p["hop"].default, p["LPF"].default, p["CUTOFF"].default, p["model"].default, p["save_wavs"].default) == \
        (0, None, False, 50, "last_trained_model", False)


def test_built_library_exports_the_sweep_and_says_109():
    lib = ctypes.CDLL(build.build_library())
    assert hasattr(lib, "f2_eval_noise_sweep")
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() >= 109


# ---- EvaluateNoiseSweep against a stub context ------------------------------------------------------------------------------
RADIUS = 5


class StubContext:
    """Stands in for the device: labels window j of level l of file b as (j + l + b) % 2 == 0, counts like the tally, says
    sigma = l + 1 + b / 16 for level l of file b (0 for the clean level) and, asked for the noisy waveforms, returns level l as the
    clean samples times l + 1."""

    def __init__(self):
        self.calls = []

    def cnn_create(self, tensors, rows, channels):
        return 1

    def eval_noise_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, snr_db, seed,
                         noisy, scores, labels, mem_space):
        K = len(snr_db)
        lengths = np.diff(offsets)
        self.calls.append(dict(B=B, lengths=lengths.tolist(), dtype=wave_dtype, Cn=Cn, hop=hop, step=step, lpf=lpf, cutoff=cutoff,
                               snr=list(snr_db), seed=seed, noisy=noisy is not None))
        assert handle == 1 and scores is None and mem_space == _lib.MEM_HOST and wave.shape[0] == offsets[-1]
        per = [_lib.strided_window_count(int(n), radius, step, hop) for n in lengths] * (K + 1)
        wo = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        assert labels.shape == (wo[-1],)
        for u in range((K + 1) * B):
            l, b = divmod(u, B)
            labels[wo[u]:wo[u + 1]] = (np.arange(per[u]) + l + b) % 2 == 0
        if noisy is not None:
            assert noisy.shape == ((K + 1) * offsets[-1],) and noisy.dtype == np.float64
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


def write_wavs(workdir, lengths, rate=16000, dtype=np.int16):
    from scipy.io import wavfile
    files = []
    rng = np.random.default_rng(3)
    for i, n in enumerate(lengths):
        path = str(workdir / "F{}_{}_{}.WAV".format(rate, np.dtype(dtype).name, i))
        wavfile.write(path, rate, (rng.standard_normal(n) * 3000).astype(dtype))
        files.append(path)
    return files


def printed_block(file, names, n, b, out, notice=""):
    """what the sweep prints for file b of its pass, n windows per level: the stub's labels give the counts"""
    text = "File:\t\t{}\n".format(file) + notice
    clean = (np.arange(n) + len(names) - 1 + b) % 2 == 0
    for l, name in enumerate(names):
        mine = (np.arange(n) + l + b) % 2 == 0
        text += "\tSNR {:>8}\t{} windows\t{} rising\tagreement with clean {:.4f}\n".format(name, n, mine.sum(), (mine == clean).sum() / n)
    return text + "\t\t{}\tdone ! -> {}\n".format(file, out)


def test_evaluate_noise_sweep_groups_and_writes(workdir, capsys):
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    lengths = [2000 + 7 * i for i in range(18)]
    files = write_wavs(workdir, lengths) + write_wavs(workdir, [2500], rate=8000)
    stub = StubContext()
    res = Evaluating.EvaluateNoiseSweep(files, [10, -3.5], seed=7, hop=160, model=F2CNNModel.glorot(7), ctx=stub)
    # one rate per pass, 16 files at the most
    assert [c["B"] for c in stub.calls] == [16, 2, 1]
    assert stub.calls[0]["lengths"] == lengths[:16] and stub.calls[1]["lengths"] == lengths[16:] and stub.calls[2]["lengths"] == [2500]
    assert [c["step"] for c in stub.calls] == [160, 160, 80]
    assert all(c["snr"] == [10.0, -3.5] and c["hop"] == 160 and c["seed"] == 7 and not c["lpf"] and c["cutoff"] == 0.0 and not c["noisy"]
               for c in stub.calls)
    assert list(res) == files
    K = 2
    expected = ""
    for i, file in enumerate(files):
        stem = os.path.basename(os.path.splitext(file)[0])
        out = os.path.join("OutputWavFiles", "addedNoise", stem + ".sweep.npz")
        archive = np.load(out)
        assert list(archive.files) == ["snr_db", "sigma", "windows", "rising", "agree", "agreement", "seed", "hop", "labels_0", "labels_1",
                                       "labels_clean"]
        saved = dict(archive)
        assert list(res[file]) == list(archive.files)
        rate, n_samples = (16000, lengths[i]) if i < 18 else (8000, 2500)
        n = _lib.strided_window_count(n_samples, RADIUS, rate // 100, 160)
        b = i % 16 if i < 18 else 0
        assert saved["windows"].tolist() == [n] * (K + 1) and saved["windows"].dtype == np.int64
        assert saved["hop"].dtype == np.int64 and int(saved["hop"]) == 160 and saved["seed"].dtype == np.uint64 and int(saved["seed"]) == 7
        assert saved["snr_db"].tolist() == [10.0, -3.5] and saved["sigma"].tolist() == [1 + b / 16.0, 2 + b / 16.0, 0.0]
        for l, key in enumerate(("labels_0", "labels_1", "labels_clean")):
            assert saved[key].dtype == np.uint8 and np.array_equal(saved[key], (np.arange(n) + l + b) % 2 == 0), (i, key)
            assert saved["rising"][l] == saved[key].sum() and saved["agree"][l] == (saved[key] == saved["labels_clean"]).sum()
            assert np.array_equal(res[file][key], saved[key])
        assert saved["agreement"].tolist() == [1.0, 0.0, 1.0]
        expected += printed_block(file, ["10dB", "-3.5dB", "clean"], n, b, out)
    assert capsys.readouterr().out == expected
    assert sorted(os.listdir(os.path.join("OutputWavFiles", "addedNoise"))) == sorted(
        os.path.basename(os.path.splitext(f)[0]) + ".sweep.npz" for f in files)             # no WAV without save_wavs


def test_saved_wavs_low_pass_and_missing_side_files(workdir, capsys):
    from scipy.io import wavfile
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    file, = write_wavs(workdir, [2600])
    open(os.path.splitext(file)[0] + ".WRD", "w").write("0 10 x\n")                        # no .PHN, no .FB: no reference labels
    stub = StubContext()
    res = Evaluating.EvaluateNoiseSweep(file, [20, 2.5], seed=-1, LPF=True, CUTOFF=40, save_wavs=True, model=F2CNNModel.glorot(7),
                                        ctx=stub, accuracy="reference", resample=True)[file]
    call, = stub.calls
    assert call["lpf"] and call["cutoff"] == 40 and call["noisy"] and call["hop"] == 1 and call["seed"] == -1
    stem = os.path.basename(os.path.splitext(file)[0])
    out = os.path.join("OutputWavFiles", "addedNoise", stem + ".sweep.npz")
    archive = np.load(out)
    assert list(archive.files) == list(res) == ["snr_db", "sigma", "windows", "rising", "agree", "agreement", "seed", "hop", "framerate",
                                                "source_framerate", "labels_0", "labels_1", "labels_clean"]
    assert int(archive["seed"]) == 2 ** 64 - 1 and int(archive["framerate"]) == int(archive["source_framerate"]) == 16000
    n = _lib.strided_window_count(2600, RADIUS, 160, 1)
    assert archive["windows"].tolist() == [n] * 3
    clean = wavfile.read(file)[1].astype(np.float64)
    for l, name in enumerate(("20.0dB", "2.5dB")):                                       # (named as EvaluateWithNoise names them)
        target = os.path.join("OutputWavFiles", "addedNoise", stem + name)
        rate, data = wavfile.read(target + ".WAV")
        assert rate == 16000 and np.array_equal(data, clean * (l + 1))
        assert os.path.exists(target + ".WRD") and not os.path.exists(target + ".PHN") and not os.path.exists(target + ".FB")
    assert sorted(os.listdir(os.path.join("OutputWavFiles", "addedNoise"))) == sorted(
        [stem + ".sweep.npz"] + [stem + name + ext for name in ("20.0dB", "2.5dB") for ext in (".WAV", ".WRD")])
    notice = "\t\t{}\tno labels from .FB / .PHN side files: no accuracy\n".format(file)
    # (the label reader says what it misses when the pass looks for the labels, before the first file's lines)
    assert capsys.readouterr().out == "No .FB formant data file.\n" + printed_block(file, ["20dB", "2.5dB", "clean"], n, 0, out, notice)


@pytest.mark.parametrize("bad", [[], [float("nan")], [3, float("inf")]])
def test_bad_levels_are_refused_before_anything_is_read(bad):
    from f2cnn_amd.scripts.CNN import Evaluating
    with pytest.raises(ValueError, match="at least one finite SNR"):
        Evaluating.EvaluateNoiseSweep(["does-not-exist.WAV"], bad, ctx=StubContext())
