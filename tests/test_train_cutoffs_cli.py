"""Training across envelope cutoffs, the parts that need no GPU: the command line takes `--augment-cutoffs` on
`train --engine hip --from-wav` alone, never beside `--lpf`, and hands it down only when given; the epochs' cutoffs come from a
generator of their own; bad cutoffs are refused before a file is read; the three C entry points are in the built library, declared
and bound, and the stage sits where the header says."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, build, cli

NAMES = {"f2_lowpass_pick": 10, "f2_input_batch_filtered": 41, "f2_trainer_render_filtered": 25}


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


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_parser_values():
    args = cli.build_parser().parse_args(["cnn", "train", "--engine", "hip", "--from-wav", "--augment-cutoffs", "5,10,20,50", "--seed", "4"])
    assert args.augment_cutoffs == [5.0, 10.0, 20.0, 50.0] and args.seed == 4
    assert cli.augment_cutoffs_argument("0.5") == [0.5] and len(cli.augment_cutoffs_argument(",".join(["7"] * 64))) == 64
    for argv in (["cnn", "train", "--engine", "hip", "--from-wav", "--augment-snrs", "3"], ["cnn", "lpfsweep", "--file", "a.WAV", "--cutoffs", "5"],
                 ["cnn", "eval", "--file", "a.WAV"]):
        assert "augment_cutoffs" not in vars(cli.build_parser().parse_args(argv)), argv
    for word in ("--augment-cutoffs 5,10,20,50", "lpfsweep", "not with"):
        assert word in cli.__doc__, word


@pytest.mark.parametrize("bad", ["", "5,,10", "x", "0", "8000", "-3", "nan", "inf", ",".join(["7"] * 65)])
def test_parser_refuses_malformed_lists(bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "train", "--engine", "hip", "--from-wav", "--augment-cutoffs=" + bad])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--augment-cutoffs" in err and "--cutoffs takes" not in err.replace("--augment-cutoffs", "")


def test_train_hands_its_cutoffs_down_only_when_given(no_work, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    open("labels.csv", "w").write("x\n")
    base = ["cnn", "train", "--engine", "hip", "--from-wav", "--label", "labels.csv"]
    assert cli.main(base + ["--augment-cutoffs", "5,10,20,50", "--seed", "2"]) == 0
    (name, a, kw), = no_work
    assert name == "TrainFromWav" and a == () and kw == dict(labelFile="labels.csv", LPF=False, CUTOFF=None, snrs=(), seed=2,
                                                             cutoffs=(5.0, 10.0, 20.0, 50.0))
    del no_work[:]
    assert cli.main(base + ["--augment-cutoffs", "7", "--augment-snrs", "20,10", "--augment-colours", "pink", "--augment-t60", "0.3",
                            "--augment-spreads", "1", "--augment-bands", "8", "--augment-maskers", "a.wav", "--augment-masker-snrs", "3"]) == 0
    (name, a, kw), = no_work
    assert kw["cutoffs"] == (7.0,) and kw["snrs"] == (20.0, 10.0) and kw["colours"] == ("pink",) and kw["t60s"] == (0.3,)
    assert kw["bands"] == (8,) and kw["maskers"] == ("a.wav",) and kw["LPF"] is False
    del no_work[:]
    # without the option the calls are the ones they were: no keyword of the new stage
    for rest in ([], ["--augment-snrs", "3"], ["--lpf", "50"], ["--augment-maskers", "a.wav", "--augment-masker-snrs", "3"]):
        assert cli.main(base + rest) == 0
        assert "cutoffs" not in no_work[-1][2], rest
    assert no_work[2][2]["LPF"] is True


def test_refusals_touch_nothing(no_work, capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    open("labels.csv", "w").write("x\n")
    base = ["cnn", "train", "--engine", "hip", "--from-wav", "--label", "labels.csv"]
    opt = ["--augment-cutoffs", "5,50"]
    for argv, words in ((["cnn", "train"] + opt, ("--augment-cutoffs", "--engine hip")),
                        (["cnn", "train", "--engine", "torch"] + opt, ("--augment-cutoffs", "--engine hip")),
                        (["cnn", "train", "--engine", "hip"] + opt, ("--augment-cutoffs", "--from-wav")),
                        (base + opt + ["--lpf", "50"], ("--augment-cutoffs", "--lpf")),
                        (["cnn", "eval", "--file", "a.WAV"] + opt, ("--augment-cutoffs", "only applies to 'cnn train'")),
                        (["cnn", "lpfsweep", "--file", "a.WAV", "--cutoffs", "5"] + opt, ("--augment-cutoffs", "only applies to 'cnn train'")),
                        (["cnn", "test"] + opt, ("--augment-cutoffs", "only applies to 'cnn train'"))):
        assert cli.main(argv) == 1, argv
        out = capsys.readouterr().out
        assert all(w in out for w in words), (argv, out)
    assert no_work == [] and os.listdir(".") == ["labels.csv"]


# ---- the epochs' cutoffs ----------------------------------------------------------------------------------------------------
def test_the_cutoff_generator_is_its_own():
    from f2cnn_amd.scripts.CNN import Training
    seed, B = 11, 9
    streams = (Training.NOISE_STREAM, Training.ROOM_STREAM, Training.SMEAR_STREAM, Training.MASKER_STREAM)
    assert Training.CUTOFF_STREAM == 0x6375746F and Training.CUTOFF_STREAM not in streams and len(set(streams)) == 4

    def others(rngs):
        return (Training.draw_epoch_noise(rngs[0], 3, B), Training.draw_epoch_rooms(rngs[1], 2, B), Training.draw_epoch_smear(rngs[2], 4, B),
                Training.draw_epoch_maskers(rngs[3], 6, B))
    plain = [np.random.default_rng([seed, s]) for s in streams]
    mixed = [np.random.default_rng([seed, s]) for s in streams]
    rng = np.random.default_rng([seed, Training.CUTOFF_STREAM])
    seen = []
    for _ in range(3):
        want = others(plain)
        cutoff_of = Training.draw_epoch_cutoffs(rng, 4, B)
        got = others(mixed)
        assert cutoff_of.dtype == np.int32 and cutoff_of.shape == (B,) and 0 <= cutoff_of.min() and cutoff_of.max() <= 4
        seen.append(cutoff_of)
        for w, g in zip(want, got):
            if isinstance(w, tuple):
                assert np.array_equal(w[0], g[0]) and w[1] == g[1]
            else:
                assert np.array_equal(w, g)
    assert len({tuple(s) for s in seen}) == 3 and 4 in np.concatenate(seen)
    again = Training.draw_epoch_cutoffs(np.random.default_rng([seed, Training.CUTOFF_STREAM]), 4, B)
    assert np.array_equal(again, seen[0])
    # drawn like draw_epoch_smear: the same numbers from the same generator state
    assert np.array_equal(Training.draw_epoch_cutoffs(np.random.default_rng(5), 4, B), Training.draw_epoch_smear(np.random.default_rng(5), 4, B))


def test_bad_cutoffs_are_refused_before_a_file_is_read(tmp_path, monkeypatch):
    from f2cnn_amd import config
    from f2cnn_amd.scripts.CNN import Training
    monkeypatch.chdir(tmp_path)
    config.write_default()
    for kw, word in ((dict(cutoffs=(5.0, 0.0)), "outside"), (dict(cutoffs=(8000.0,)), "8000"), (dict(cutoffs=(float("nan"),)), "outside"),
                     (dict(cutoffs=(float("inf"),)), "outside"), (dict(cutoffs=(-1.0,)), "outside"), (dict(cutoffs=(7.0,) * 65), "at most 64"),
                     (dict(cutoffs=(5.0,), LPF=True, CUTOFF=50), "LPF")):
        with pytest.raises(ValueError, match=word):
            Training.TrainFromWav(labelFile="does-not-exist.csv", seed=1, **kw)
    assert Training.check_cutoffs([5, "10"]) == (5.0, 10.0) and Training.check_cutoffs(()) == ()
    assert Training.MAX_CUTOFFS == cli.NOISE_LEVELS_MAX == 64


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
    stage = ["const double* cutoff_levels_hz", "int Kc", "const int32_t* cutoff_of"]
    masked = params("f2_input_batch_masked")
    assert params("f2_input_batch_filtered") == masked[:-2] + stage + masked[-2:]
    assert params("f2_trainer_render_filtered") == params("f2_trainer_render_masked") + stage
    assert params("f2_lowpass_pick") == ["f2_ctx* ctx", "const double* env", "const int64_t* offsets", "int B", "int C", "const double* cutoff_hz",
                                         "int K", "const int32_t* cutoff_of", "double* filtered", "int mem_space"]
    # the bindings follow the declarations argument by argument: the stage's three land where the header puts them
    sig = _lib.SIGNATURES
    assert sig["f2_input_batch_filtered"][1] == sig["f2_input_batch_masked"][1][:-2] + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p] + \
        sig["f2_input_batch_masked"][1][-2:]
    assert sig["f2_trainer_render_filtered"][1] == sig["f2_trainer_render_masked"][1] + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert _lib._STAGE_KEYS["filtered"] == _lib._STAGE_KEYS["masked"] + ["cutoff_levels_hz", "Kc", "cutoff_of"]
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() == 115
    for word in ("f2_version\n * stays 115 with these three entries", "F2_ERR_UNSUPPORTED", "lpf = 1 is F2_ERR_INVALID"):
        assert word in text, word
    internal = open(os.path.join(ROOT, "f2cnn_amd", "csrc", "f2_internal.h")).read()
    assert int(re.search(r"^#define\s+F2_LOWPASS_MAX_CUTOFFS\s+(\d+)\s*$", internal, flags=re.M).group(1)) == 64


def test_signature_defaults():
    from f2cnn_amd.scripts.CNN import Training
    from f2cnn_amd.trainer import Trainer
    for fn in (Trainer.render, Trainer.render_wet):
        p = inspect.signature(fn).parameters
        assert p["cutoffs"].default is None and p["cutoff_of"].default is None
        assert list(p)[-2:] == ["cutoffs", "cutoff_of"]                      # behind everything that was there
    p = inspect.signature(_lib.Context.trainer_render_filtered).parameters
    assert p["cutoffs"].default == () and p["cutoff_of"].default is None
    p = inspect.signature(Training.TrainFromWav).parameters
    assert p["cutoffs"].default == () and list(p)[-1] == "cutoffs"
    assert inspect.signature(Training._render_windows).parameters["cutoff"].default is None


def test_stage_arguments_are_marshalled_in_the_order_of_the_declaration():
    v = dict(snr_db=(), level_of=None, seed=0, firs=None, rirs=(), room_of=None, mixes=None, mix_of=None, channels=4, maskers=None,
             masker_of=None, masker_snrs=(), masker_level_of=None, cutoffs=(5, 50.0), cutoff_of=[1, 2, 0])
    keys = [k for k in _lib._STAGE_KEYS["filtered"] if k != "first_utterance"]
    args, alive = _lib._stage_args(keys, v)
    assert len(args) == NAMES["f2_trainer_render_filtered"] - 2 and args[-2] == 2       # (behind ctx and trainer)
    assert alive["cutoff_levels_hz"].dtype == np.float64 and alive["cutoff_levels_hz"].tolist() == [5.0, 50.0]
    assert alive["cutoff_of"].dtype == np.int32 and alive["cutoff_of"].tolist() == [1, 2, 0]
    assert args[-3] == alive["cutoff_levels_hz"].ctypes.data and args[-1] == alive["cutoff_of"].ctypes.data
    args, alive = _lib._stage_args(keys, dict(v, cutoffs=(), cutoff_of=None))
    assert args[-3:] == [None, 0, None]
