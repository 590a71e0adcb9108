"""Recorded maskers, the parts that need no GPU: masker.py reads the RIFF formats, mixes stereo down and refuses what cannot be a
masker; the level grid is masker-major with names like `babble 10dB`; the command line takes `--maskers` on noisesweep alone and
`--augment-maskers` / `--augment-masker-snrs` on `train --engine hip --from-wav` alone and hands them down; the epochs' maskers come
from a generator of their own; the C entry points are in the built library, declared and bound; and EvaluateNoiseSweep with maskers
groups its files and writes its .maskersweep.npz, held against a stub context that stands in for the device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
from scipy.io import wavfile

from conftest import ROOT
from f2cnn_amd import _lib, build, cli, masker

NAMES = {"f2_masker_levels": 17, "f2_eval_masker_sweep": 30, "f2_masker_pick": 19, "f2_input_batch_masked": 38, "f2_trainer_render_masked": 22}


# ---- masker.py --------------------------------------------------------------------------------------------------------------
def test_load_masker_reads_the_formats_in_int16_units(tmp_path):
    x = (np.random.default_rng(1).standard_normal(500) * 3000).astype(np.int16)
    cases = {"i16": x, "u8": ((x.astype(np.int32) >> 8) + 128).astype(np.uint8), "i32": x.astype(np.int32) << 16,
             "f32": (x / 32768.0).astype(np.float32), "f64": x / 32768.0}
    for name, data in cases.items():
        path = str(tmp_path / (name + ".wav"))
        wavfile.write(path, 16000, data)
        m = masker.LoadMasker(path, 16000)
        assert m.dtype == np.float64 and m.shape == (500,) and m.flags["C_CONTIGUOUS"]
        want = ((x.astype(np.int32) >> 8) * 256).astype(np.float64) if name == "u8" else x.astype(np.float64)
        assert np.array_equal(m, want), name
        assert np.array_equal(masker.LoadMasker(path, 16000, resample=True), want), name      # (the rate is right: nothing to resample)


def test_load_masker_mixes_stereo_down_and_names_both_rates(tmp_path):
    left = (np.arange(300) % 50 * 100).astype(np.int16)
    right = (-(np.arange(300) % 30) * 50).astype(np.int16)
    path = str(tmp_path / "cafe.wav")
    wavfile.write(path, 16000, np.stack([left, right], axis=1))
    assert np.array_equal(masker.LoadMasker(path, 16000), (left.astype(np.float64) + right) / 2)
    assert masker.MaskerName(path) == "cafe" and masker.MaskerName("a/b/babble.WAV") == "babble"
    with pytest.raises(ValueError) as e:
        masker.LoadMasker(path, 8000)
    assert "16000 Hz" in str(e.value) and "8000 Hz" in str(e.value) and "cafe.wav" in str(e.value)


def test_load_masker_refuses_what_cannot_mask(tmp_path):
    for name, data in (("empty", np.zeros(0, np.int16)), ("silent", np.zeros(100, np.int16)),
                       ("nan", np.array([0.1, np.nan, 0.2], np.float32)), ("inf", np.array([0.1, np.inf], np.float64))):
        path = str(tmp_path / (name + ".wav"))
        wavfile.write(path, 16000, data)
        with pytest.raises(ValueError, match=name + ".wav"):
            masker.LoadMasker(path, 16000)


def test_the_level_grid_is_masker_major():
    grid = masker.MaskerLevels(["/x/babble.wav", "cafe.WAV"], [10.0, -3.5, 0])
    assert grid == [(0, "babble", 10.0), (0, "babble", -3.5), (0, "babble", 0.0), (1, "cafe", 10.0), (1, "cafe", -3.5), (1, "cafe", 0.0)]
    assert masker.MaskerLevels("a.wav,b.wav", [5]) == [(0, "a", 5.0), (1, "b", 5.0)]
    assert len(masker.MaskerLevels(["m.wav"] * 8, range(8))) == 64 and len(masker.MaskerLevels(["m.wav"] * 64, [0])) == 64
    for maskers, snrs in (([], [3.0]), (["a.wav", ""], [3.0]), (["a.wav"], []), (["a.wav"] * 5, range(13)), (["a.wav"] * 65, [0])):
        with pytest.raises(ValueError):
            masker.MaskerLevels(maskers, snrs)
    assert masker.MAX_LEVELS == cli.NOISE_LEVELS_MAX == 64 and masker.MAX_RECORDINGS == cli.MASKER_RECORDINGS_MAX == 64


# ---- the command line -------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_work(monkeypatch):
    """any evaluation or training the command line would start is recorded, not run"""
    from f2cnn_amd.scripts.CNN import Evaluating, Training
    seen = []
    for name in ("EvaluateReverbSweep", "EvaluateCutoffSweep", "EvaluateSmearSweep", "EvaluateNoiseSweep", "EvaluateOneWavFile",
                 "EvaluateWithNoise", "EvaluateRandom"):
        monkeypatch.setattr(Evaluating, name, lambda *a, _name=name, **kw: seen.append((_name, a, kw)))
    for name in ("TrainFromWav", "TrainAndPlotLoss"):
        monkeypatch.setattr(Training, name, lambda *a, _name=name, **kw: seen.append((_name, a, kw)))
    return seen


def test_sweep_parses_and_hands_its_maskers_down(no_work):
    args = cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "20,10,0", "--maskers", "babble.wav,cafe.wav",
                                          "--seed", "4", "--hop", "frame", "--accuracy", "--resample", "--save-wavs"])
    assert args.maskers == ["babble.wav", "cafe.wav"] and args.snrs == [20.0, 10.0, 0.0] and args.seed == 4 and args.save_wavs
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "20,0", "--maskers", "babble.wav,cafe.wav", "--seed", "3"]) == 0
    (name, a, kw), = no_work
    assert name == "EvaluateNoiseSweep" and a == (["a.WAV"], [20.0, 0.0]) and kw == dict(seed=3, save_wavs=False, maskers=["babble.wav", "cafe.wav"])
    for word in ("--maskers", "maskersweep.npz", "babble 10dB", "--augment-maskers", "--augment-masker-snrs"):
        assert word in cli.__doc__, word


def test_without_the_options_the_commands_parse_and_call_as_before(no_work):
    for argv in (["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3"], ["cnn", "eval", "--file", "a.WAV"],
                 ["cnn", "train", "--engine", "hip", "--from-wav", "--augment-snrs", "3"]):
        assert not {"maskers", "augment_maskers", "augment_masker_snrs"} & set(vars(cli.build_parser().parse_args(argv))), argv
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3,0", "--colours", "pink"]) == 0
    (name, a, kw), = no_work
    assert kw == dict(seed=0, save_wavs=False, colours=["pink"])


@pytest.mark.parametrize("bad", ["", "a.wav,,b.wav", ",".join(["m.wav"] * 65)])
def test_parser_refuses_malformed_lists(bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3", "--maskers=" + bad])
    assert e.value.code == 2 and "--maskers" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["cnn", "train", "--augment-masker-snrs=x"])


def test_maskers_and_colours_exclude_each_other_and_need_levels(no_work, capsys):
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3", "--maskers", "b.wav", "--colours", "pink"]) == 1
    assert "--maskers and --colours" in capsys.readouterr().out
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--maskers", "b.wav"]) == 1
    assert capsys.readouterr().out.startswith("Please use --snrs")
    snrs = ",".join(str(v) for v in range(13))
    assert cli.main(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", snrs, "--maskers", "a.wav,b.wav,c.wav,d.wav,e.wav"]) == 1
    assert "5 maskers x 13 SNRs = 65" in capsys.readouterr().out
    assert no_work == []


@pytest.mark.parametrize("command,rest", [("eval", []), ("evalnoise", ["--noise", "3"]), ("evalrand", []), ("train", []), ("test", []),
                                          ("lpfsweep", ["--cutoffs", "5"]), ("reverbsweep", ["--t60", "0.2"]), ("smearsweep", ["--spreads", "1"])])
def test_the_other_commands_refuse_maskers(no_work, capsys, command, rest):
    assert cli.main(["cnn", command, "--file", "a.WAV"] + rest + ["--maskers", "b.wav"]) == 1
    out = capsys.readouterr().out
    assert "--maskers" in out and "noisesweep" in out and no_work == []


def test_train_hands_its_maskers_down_and_refuses_them_elsewhere(no_work, capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    open("labels.csv", "w").write("x\n")
    base = ["cnn", "train", "--engine", "hip", "--from-wav", "--label", "labels.csv"]
    assert cli.main(base + ["--augment-maskers", "a.wav,b.wav", "--augment-masker-snrs", "20,10,5", "--seed", "2"]) == 0
    (name, a, kw), = no_work
    assert name == "TrainFromWav" and kw["maskers"] == ("a.wav", "b.wav") and kw["masker_snrs"] == (20.0, 10.0, 5.0) and kw["snrs"] == ()
    del no_work[:]
    assert cli.main(base + ["--augment-maskers", "a.wav", "--augment-masker-snrs", "3", "--augment-snrs", "20,10", "--augment-colours", "pink",
                            "--augment-t60", "0.3", "--augment-spreads", "1", "--augment-bands", "8"]) == 0
    (name, a, kw), = no_work
    assert kw["maskers"] == ("a.wav",) and kw["snrs"] == (20.0, 10.0) and kw["colours"] == ("pink",) and kw["t60s"] == (0.3,) and kw["bands"] == (8,)
    del no_work[:]
    assert cli.main(base + ["--augment-snrs", "3"]) == 0
    assert "maskers" not in no_work[0][2]
    del no_work[:]
    for argv, word in ((["cnn", "train", "--augment-maskers", "a.wav", "--augment-masker-snrs", "3"], "--engine hip"),
                       (["cnn", "train", "--engine", "torch", "--augment-maskers", "a.wav", "--augment-masker-snrs", "3"], "--engine hip"),
                       (["cnn", "train", "--engine", "hip", "--augment-maskers", "a.wav", "--augment-masker-snrs", "3"], "--from-wav"),
                       (base + ["--augment-maskers", "a.wav"], "needs --augment-masker-snrs"),
                       (base + ["--augment-masker-snrs", "3"], "belongs to --augment-maskers"),
                       (base + ["--augment-maskers", "a.wav,b.wav,c.wav,d.wav,e.wav", "--augment-masker-snrs", ",".join(map(str, range(13)))],
                        "5 maskers x 13 SNRs = 65"),
                       (["cnn", "eval", "--file", "a.WAV", "--augment-maskers", "a.wav"], "only applies to 'cnn train'")):
        assert cli.main(argv) == 1, argv
        assert word in capsys.readouterr().out, argv
    assert no_work == []


# ---- the epochs' maskers ----------------------------------------------------------------------------------------------------
def test_the_masker_generator_is_its_own():
    from f2cnn_amd.scripts.CNN import Training
    seed, B = 11, 9
    streams = (Training.NOISE_STREAM, Training.ROOM_STREAM, Training.SMEAR_STREAM)
    assert Training.MASKER_STREAM == 0x6D61736B and Training.MASKER_STREAM not in streams

    def others(rngs):
        return (Training.draw_epoch_noise(rngs[0], 3, B), Training.draw_epoch_rooms(rngs[1], 2, B), Training.draw_epoch_smear(rngs[2], 4, B))
    plain = [np.random.default_rng([seed, s]) for s in streams]
    mixed = [np.random.default_rng([seed, s]) for s in streams]
    rng = np.random.default_rng([seed, Training.MASKER_STREAM])
    seen = []
    for _ in range(3):
        want = others(plain)
        level_of, masker_seed = Training.draw_epoch_maskers(rng, 6, B)
        got = others(mixed)
        assert level_of.dtype == np.int32 and level_of.shape == (B,) and 0 <= level_of.min() and level_of.max() <= 6 and 0 <= masker_seed < 2 ** 63
        seen.append(level_of)
        for w, g in zip(want, got):
            if isinstance(w, tuple):
                assert np.array_equal(w[0], g[0]) and w[1] == g[1]
            else:
                assert np.array_equal(w, g)
    assert len({tuple(s) for s in seen}) == 3 and 6 in np.concatenate(seen)
    again = Training.draw_epoch_maskers(np.random.default_rng([seed, Training.MASKER_STREAM]), 6, B)
    assert np.array_equal(again[0], seen[0])
    sig = inspect.signature(Training.TrainFromWav).parameters
    assert sig["maskers"].default == () and sig["masker_snrs"].default == ()


# ---- the C entry points -----------------------------------------------------------------------------------------------------
def test_entries_are_in_the_library_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(build.build_library())
    for name, n in NAMES.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name + " is not declared in include/f2cnn_hip.h"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")) == n, name
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code).group(1).split(",")]
    stage = ["const double* masker_snr_db", "const double* masker", "const int64_t* masker_offsets", "int R", "const int32_t* masker_of", "int Kk",
             "const int32_t* masker_level_of"]
    smeared = params("f2_input_batch_smeared")
    assert params("f2_input_batch_masked") == smeared[:-2] + stage + smeared[-2:]
    assert params("f2_trainer_render_masked") == params("f2_trainer_render_smeared") + stage
    assert params("f2_masker_levels") == ["f2_ctx* ctx", "const void* wave", "int wave_dtype", "const int64_t* offsets", "int B",
                                          "const double* snr_db", "const double* masker", "const int64_t* masker_offsets", "int R",
                                          "const int32_t* masker_of", "int K", "uint64_t seed", "double* noisy", "double* sigma_or_null",
                                          "double* gain_or_null", "int64_t* start_or_null", "int mem_space"]
    assert _lib.SIGNATURES["f2_masker_levels"][1][11] is ctypes.c_uint64 and _lib.SIGNATURES["f2_masker_pick"][1][12] is ctypes.c_uint32
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() == 115
    for word in ("0x4D41534B", "gain = sigma / sqrt(P / n)", "F2_ERR_UNSUPPORTED", "f2_version stays 115"):
        assert word in text, word
    internal = open(os.path.join(ROOT, "f2cnn_amd", "csrc", "f2_internal.h")).read()
    define = lambda name: int(re.search(r"^#define\s+" + name + r"\s+(\d+)\s*$", internal, flags=re.M).group(1))
    assert _lib.MASKER_MAX_RECORDINGS == define("F2_MASKER_MAX_RECORDINGS") == 64 and _lib.MASKER_MAX_LEVELS == define("F2_MASKER_MAX_LEVELS") == 64
    assert _lib.MASKER_MAX_SAMPLES == 1 << 26 and "(int64_t(1) << 26)" in internal and _lib.MASKER_STREAM == 0x4D41534B
    from f2cnn_amd.trainer import Trainer
    for fn in (Trainer.render, Trainer.render_wet, _lib.Context.trainer_render_masked):
        p = inspect.signature(fn).parameters
        assert p["maskers"].default is None and p["masker_level_of"].default is None
    from f2cnn_amd.scripts.CNN import Evaluating
    p = inspect.signature(Evaluating.EvaluateNoiseSweep).parameters
    assert p["maskers"].default is None


def test_pack_maskers_wants_a_recording_per_level():
    samples, moff, mof = _lib._maskers([np.ones(2), [0.5, 0.25, 4.0]], (1, 0, 1), 3)
    assert samples.tolist() == [1.0, 1.0, 0.5, 0.25, 4.0] and moff.tolist() == [0, 2, 5] and mof.tolist() == [1, 0, 1] and mof.dtype == np.int32
    assert _lib._maskers(None, None, 0) == (None, None, None)
    with pytest.raises(ValueError, match="one per level"):
        _lib._maskers([np.ones(2)], (0,), 2)


# ---- EvaluateNoiseSweep(maskers=...) against a stub context -----------------------------------------------------------------
RADIUS = 5


class StubContext:
    """Stands in for the device: labels window j of level l of file b as (j + l + b) % 2 == 0, counts like the tally, says
    sigma = l + 1 + b / 16, gain = sigma / 4 and start = 100 l + b for level l of file b (0 for the clean level) and, asked for the
    noisy waveforms, returns level l as the clean samples times l + 1. It has no other sweep: a call of one is an AttributeError."""

    def __init__(self):
        self.calls = []

    def cnn_create(self, tensors, rows, channels):
        return 1

    def eval_masker_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, snr_db, maskers,
                          masker_of, seed, noisy, scores, labels, mem_space):
        K = len(snr_db)
        lengths = np.diff(offsets)
        self.calls.append(dict(B=B, step=step, hop=hop, lpf=lpf, snr=list(snr_db), seed=seed, maskers=[np.array(m) for m in maskers],
                               masker_of=list(masker_of), noisy=noisy is not None))
        assert handle == 1 and scores is None and mem_space == _lib.MEM_HOST and wave.shape[0] == offsets[-1] and len(masker_of) == K
        per = [_lib.strided_window_count(int(n), radius, step, hop) for n in lengths] * (K + 1)
        wo = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
        for u in range((K + 1) * B):
            l, b = divmod(u, B)
            labels[wo[u]:wo[u + 1]] = (np.arange(per[u]) + l + b) % 2 == 0
        if noisy is not None:
            for l in range(K + 1):
                noisy[l * offsets[-1]:(l + 1) * offsets[-1]] = wave.astype(np.float64) * (l + 1)
        sigma = np.array([(l + 1 + b / 16.0) if l < K else 0.0 for l in range(K + 1) for b in range(B)])
        start = np.array([(100 * l + b) if l < K else 0 for l in range(K + 1) for b in range(B)], np.int64)
        stats = np.zeros(((K + 1) * B, 2), np.int64)
        for u in range((K + 1) * B):
            mine, ref = labels[wo[u]:wo[u + 1]], labels[wo[K * B + u % B]:wo[K * B + u % B + 1]]
            stats[u] = mine.sum(), (mine == ref).sum()
        return wo, sigma, stats, sigma / 4, start


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    from f2cnn_amd import config
    monkeypatch.chdir(tmp_path)
    config.write_default()
    return tmp_path


def write_wavs(workdir, lengths, rate=16000, stem="F"):
    files = []
    rng = np.random.default_rng(3)
    for i, n in enumerate(lengths):
        path = str(workdir / "{}{}_{}.WAV".format(stem, rate, i))
        wavfile.write(path, rate, (rng.standard_normal(n) * 3000).astype(np.int16))
        files.append(path)
    return files


def test_evaluate_masker_sweep_groups_names_and_writes(workdir, capsys):
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    lengths = [2000 + 7 * i for i in range(17)]
    files = write_wavs(workdir, lengths)
    babble, cafe = write_wavs(workdir, [700, 1300], stem="noise")
    stub = StubContext()
    res = Evaluating.EvaluateNoiseSweep(files, [10, -3.5], seed=7, hop=160, model=F2CNNModel.glorot(7), ctx=stub, maskers=[babble, cafe],
                                        save_wavs=False)
    K = 4
    assert [c["B"] for c in stub.calls] == [16, 1]
    for c in stub.calls:
        assert c["snr"] == [10.0, -3.5] * 2 and c["masker_of"] == [0, 0, 1, 1] and c["seed"] == 7 and not c["noisy"]
        assert [len(m) for m in c["maskers"]] == [700, 1300] and np.array_equal(c["maskers"][0], wavfile.read(babble)[1].astype(np.float64))
    names = ["noise16000_0 10dB", "noise16000_0 -3.5dB", "noise16000_1 10dB", "noise16000_1 -3.5dB", "clean"]
    expected = ""
    for i, file in enumerate(files):
        stem = os.path.basename(os.path.splitext(file)[0])
        out = os.path.join("OutputWavFiles", "addedNoise", stem + ".maskersweep.npz")
        archive = np.load(out)
        assert list(archive.files) == list(res[file]) == ["snr_db", "maskers", "masker_files", "sigma", "gain", "start", "windows", "rising",
                                                          "agree", "agreement", "seed", "hop"] + ["labels_%d" % k for k in range(K)] + ["labels_clean"]
        saved = dict(archive)
        n = _lib.strided_window_count(lengths[i], RADIUS, 160, 160)
        b = i % 16
        assert saved["windows"].tolist() == [n] * (K + 1) and int(saved["hop"]) == 160 and int(saved["seed"]) == 7
        assert saved["snr_db"].tolist() == [10.0, -3.5] * 2 and saved["sigma"].tolist() == [l + 1 + b / 16.0 for l in range(K)] + [0.0]
        assert saved["gain"].tolist() == [(l + 1 + b / 16.0) / 4 for l in range(K)] + [0.0]
        assert saved["start"].tolist() == [100 * l + b for l in range(K)] + [0] and saved["start"].dtype == np.int64
        assert saved["maskers"].tolist() == ["noise16000_0"] * 2 + ["noise16000_1"] * 2 and saved["masker_files"].tolist() == [babble, cafe]
        clean = (np.arange(n) + K + b) % 2 == 0
        expected += "File:\t\t{}\n".format(file)
        for l, name in enumerate(names):
            mine = (np.arange(n) + l + b) % 2 == 0
            expected += "\t{:>16}\t{} windows\t{} rising\tagreement with clean {:.4f}\n".format(name, n, mine.sum(), (mine == clean).sum() / n)
        expected += "\t\t{}\tdone ! -> {}\n".format(file, out)
    assert capsys.readouterr().out == expected
    assert sorted(os.listdir(os.path.join("OutputWavFiles", "addedNoise"))) == sorted(
        os.path.basename(os.path.splitext(f)[0]) + ".maskersweep.npz" for f in files)       # no .sweep.npz, no WAV


def test_saved_wavs_are_named_by_masker_and_level(workdir):
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Evaluating
    file, = write_wavs(workdir, [2600])
    babble, = write_wavs(workdir, [900], stem="babble")
    stub = StubContext()
    Evaluating.EvaluateNoiseSweep(file, [20, 2.5], save_wavs=True, model=F2CNNModel.glorot(7), ctx=stub, maskers=babble)
    stem = os.path.basename(os.path.splitext(file)[0])
    clean = wavfile.read(file)[1].astype(np.float64)
    names = ["_babble16000_0_20dB", "_babble16000_0_2.5dB"]
    for l, name in enumerate(names):
        rate, data = wavfile.read(os.path.join("OutputWavFiles", "addedNoise", stem + name + ".WAV"))
        assert rate == 16000 and np.array_equal(data, clean * (l + 1))
    assert sorted(os.listdir(os.path.join("OutputWavFiles", "addedNoise"))) == sorted([stem + ".maskersweep.npz"] + [stem + n + ".WAV" for n in names])


def test_bad_maskers_are_refused_before_a_file_is_read(workdir):
    from f2cnn_amd.scripts.CNN import Evaluating
    for kw in (dict(maskers=[]), dict(maskers=["a.wav", ""]), dict(maskers=["a.wav"] * 33), dict(maskers=["a.wav"], colours=["pink"])):
        with pytest.raises(ValueError):
            Evaluating.EvaluateNoiseSweep(["does-not-exist.WAV"], [3.0, 0.0], ctx=StubContext(), **kw)
    # a masker at another rate: masker.py's message, which names both rates
    file, = write_wavs(workdir, [2600])
    slow, = write_wavs(workdir, [900], rate=8000, stem="slow")
    from f2cnn_amd.model import F2CNNModel
    with pytest.raises(ValueError, match="8000 Hz"):
        Evaluating.EvaluateNoiseSweep(file, [3.0], model=F2CNNModel.glorot(7), ctx=StubContext(), maskers=[slow])
