"""`cnn train --engine hip --from-wav --augment-spreads / --augment-bands`: what the command line refuses and hands on, the order and
the names of the levels, the epoch's draw, the matrices' errors before any file is read, that the noise and room draws do not move,
and the declarations of the three entries. No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, build, cli, smear
from f2cnn_amd.gammatone import filters
from f2cnn_amd.scripts.CNN import Evaluating, Training

TRAIN = ["cnn", "train", "--engine", "hip", "--from-wav"]
WHY = "stored windows are normalised already and cannot be mixed across their channels"
REFUSALS = [(["cnn", "train", "--engine", "hip", "--augment-spreads", "1"], "--augment-spreads needs --from-wav: " + WHY),
            (["cnn", "train", "--engine", "hip", "--augment-bands", "8"], "--augment-bands needs --from-wav: " + WHY),
            (["cnn", "train", "--augment-spreads", "1", "--augment-bands", "8"], "--augment-spreads needs --engine hip"),
            (["cnn", "train", "--engine", "torch", "--augment-bands", "8"], "--augment-bands needs --engine hip"),
            (["cnn", "train", "--from-wav", "--augment-spreads", "1"], "--from-wav needs --engine hip"),
            (["cnn", "eval", "--file", "a.WAV", "--augment-spreads", "1"], "--augment-spreads only applies to 'cnn train'"),
            (["cnn", "smearsweep", "--file", "a.WAV", "--spreads", "1", "--augment-bands", "8"], "--augment-bands only applies to 'cnn train'"),
            (TRAIN + ["--augment-spreads", ",".join(str(v + 1) for v in range(60)), "--augment-bands", "1,2,3,4,5"],
             "at most 64 spectral resolutions, not 65")]


@pytest.mark.parametrize("argv,message", REFUSALS)
def test_refusals_touch_nothing(argv, message, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    called = []
    monkeypatch.setattr(Training, "TrainFromWav", lambda **kw: called.append(kw))
    monkeypatch.setattr(Training, "TrainAndPlotLoss", lambda **kw: called.append(kw))
    monkeypatch.setattr(_lib, "default_context", lambda *a, **k: pytest.fail("a refused command line opened the device"))
    assert cli.main(argv) != 0
    assert message in capsys.readouterr().out
    assert not called and os.listdir(tmp_path) == []


@pytest.mark.parametrize("flag,text,word", [("--augment-spreads", "1,-2", "takes a comma-separated list of positive spreads in ERB"),
                                            ("--augment-spreads", "", "takes a comma-separated list of positive spreads in ERB"),
                                            ("--augment-spreads", "inf", "takes a comma-separated list of positive spreads in ERB"),
                                            ("--augment-bands", "8,0", "takes a comma-separated list of positive whole numbers of bands"),
                                            ("--augment-bands", "2.5", "takes a comma-separated list of positive whole numbers of bands")])
def test_a_bad_value_is_a_usage_error(flag, text, word, capsys):
    with pytest.raises(SystemExit) as ei:
        cli.main(TRAIN + [flag, text])
    assert ei.value.code == 2 and word in capsys.readouterr().err


def test_parser_values():
    args = cli.build_parser().parse_args(TRAIN + ["--augment-spreads", "0.5,4", "--augment-bands", "16,8"])
    assert args.augment_spreads == [0.5, 4.0] and args.augment_bands == [16, 8]
    assert "spreads" not in args and "bands" not in args
    args = cli.build_parser().parse_args(TRAIN + ["--augment-snrs", "20"])
    assert "augment_spreads" not in args and "augment_bands" not in args
    assert "--augment-spreads" in cli.__doc__ and "--augment-bands" in cli.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--augment-spreads" in readme and "--augment-bands" in readme


def test_main_hands_the_levels_to_TrainFromWav(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    called = []
    monkeypatch.setattr(Training, "TrainFromWav", lambda **kw: called.append(kw))
    open("mine.csv", "w").close()
    base = TRAIN + ["-l", "mine.csv"]
    assert cli.main(base + ["--augment-spreads", "0.5,2", "--seed", "9"]) == 0
    assert called.pop() == dict(labelFile="mine.csv", LPF=False, CUTOFF=None, snrs=(), seed=9, spreads=(0.5, 2.0), bands=())
    assert cli.main(base + ["--augment-bands", "16,8", "--augment-snrs", "3", "--augment-colours", "pink", "--augment-t60", "0.3", "--augment-rirs",
                            "a.wav", "--lpf", "50"]) == 0
    assert called.pop() == dict(labelFile="mine.csv", LPF=True, CUTOFF=50, snrs=(3.0,), seed=None, t60s=(0.3,), rirs=("a.wav",), drr_db=0.0,
                                colours=("pink",), spreads=(), bands=(16, 8))
    assert cli.main(base + ["--augment-snrs", "20"]) == 0                     # without them: the call it was
    assert called.pop() == dict(labelFile="mine.csv", LPF=False, CUTOFF=None, snrs=(20.0,), seed=None)


def test_the_levels_are_the_sweeps():
    """spreads in the order given, then bands, sharp last; names and matrices those of `cnn smearsweep`"""
    freqs = filters.centre_freqs(16000, 128, 100)
    mixes, names = Training.build_smear_levels((2.0, 0.5), (16, 8), freqs)
    assert names == ["2ERB", "0.5ERB", "16bands", "8bands"] and mixes.shape == (4, 128, 128) and mixes.dtype == np.float64
    want = [smear.SmearMatrix(freqs, 2.0), smear.SmearMatrix(freqs, 0.5), smear.BandMatrix(128, 16), smear.BandMatrix(128, 8)]
    for got, w in zip(mixes, want):
        assert np.array_equal(got, w)
    assert Evaluating.SmearLevels((2.0, 0.5), (16, 8), 128)[2] == names
    assert Training.build_smear_levels((), (), freqs) == (None, [])
    assert Training.build_smear_levels((), (4,), freqs)[1] == ["4bands"]


def test_the_draw_of_an_epoch():
    """draw_epoch_smear(rng, Km, B): one level in [0, Km] per file from default_rng([seed, SMEAR_STREAM]), reproducibly"""
    assert Training.SMEAR_STREAM == 0x736D6561 == int.from_bytes(b"smea", "big")
    assert len({Training.SMEAR_STREAM, Training.NOISE_STREAM, Training.ROOM_STREAM}) == 3
    for Km in (1, 6):
        a, b = np.random.default_rng([5, Training.SMEAR_STREAM]), np.random.default_rng([5, Training.SMEAR_STREAM])
        for _ in range(3):
            mix_of = Training.draw_epoch_smear(a, Km, 40)
            assert mix_of.dtype == np.int32 and np.array_equal(mix_of, b.integers(0, Km + 1, 40).astype(np.int32))
            assert mix_of.min() >= 0 and mix_of.max() <= Km
    levels = Training.draw_epoch_smear(np.random.default_rng([5, Training.SMEAR_STREAM]), 6, 400)
    assert set(levels.tolist()) == set(range(7))


class Planned(Exception):
    pass


class FakeTrainer:
    """records what TrainFromWav asks of a trainer; the second epoch's steps end the run"""
    iterations = 0

    def __init__(self, log):
        self.log = log

    def set_waves(self, *a, **k):
        pass

    def render(self, snrs=(), level_of=None, seed=0, firs=None, mixes=None, mix_of=None):
        self.log.append(dict(level_of=level_of, seed=seed, mix_of=mix_of, mixes=mixes))

    def render_wet(self, rirs=(), room_of=None, snrs=(), level_of=None, seed=0, firs=None, mixes=None, mix_of=None):
        self.log.append(dict(room_of=room_of, level_of=level_of, seed=seed, mix_of=mix_of, mixes=mixes))

    def steps(self, order, batch):
        if len(self.log) == 2:
            raise Planned()
        return 0.0, 0

    def model(self):
        raise Planned()


def planned_run(tmp_path, monkeypatch, **kw):
    """the renders of the first two epochs of TrainFromWav on a corpus of four TRAIN files, no device"""
    import wav_corpus
    from f2cnn_amd import config
    monkeypatch.chdir(tmp_path)
    config.write_default(batch_size=16, epochs=2)
    wav_corpus.write(n_train=4, n_test=0)
    log = []
    monkeypatch.setattr(Training, "_hip_trainer", lambda rows, channels, seed, lr, decay, ctx: (FakeTrainer(log), np.random.default_rng(seed)))
    monkeypatch.setattr(Training, "_hip_validate", lambda *a, **k: pytest.fail("nothing to validate"))
    monkeypatch.setattr(Training, "_render_windows", lambda ctx, waves, centers, coefs, cfg, *a, **k: np.zeros((0, 11, 128), np.float32))
    with pytest.raises(Planned):
        Training.TrainFromWav(seed=3, verbose=0, ctx=object(), **kw)
    return log


def test_the_noise_and_room_draws_do_not_move(tmp_path, monkeypatch):
    old = planned_run(tmp_path, monkeypatch, snrs=(20.0, 0.0), t60s=(0.05,))
    new = planned_run(tmp_path, monkeypatch, snrs=(20.0, 0.0), t60s=(0.05,), spreads=(1.0,), bands=(8,))
    assert len(old) == len(new) == 2
    rng = np.random.default_rng([3, Training.SMEAR_STREAM])
    for o, n in zip(old, new):
        assert np.array_equal(o["level_of"], n["level_of"]) and o["seed"] == n["seed"] and np.array_equal(o["room_of"], n["room_of"])
        assert o["mix_of"] is None and o["mixes"] is None
        assert np.array_equal(n["mix_of"], Training.draw_epoch_smear(rng, 2, 4)) and n["mixes"].shape == (2, 128, 128)
    # the levels alone: a render per epoch all the same
    alone = planned_run(tmp_path, monkeypatch, bands=(8,))
    assert len(alone) == 2 and all(r["level_of"] is None and r["mix_of"] is not None for r in alone)


@pytest.mark.parametrize("kw,message", [(dict(spreads=(-1.0,)), "finite and positive"), (dict(spreads=(float("nan"),)), "finite and positive"),
                                        (dict(bands=(129,)), "between 1 and the 128 channels"), (dict(bands=(2.5,)), "whole number"),
                                        (dict(spreads=tuple(range(1, 61)), bands=(1, 2, 3, 4, 5)), "at most 64 levels")])
def test_matrix_errors_come_before_any_file_is_read(kw, message, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(_lib, "default_context", lambda *a, **k: pytest.fail("the device was opened"))
    monkeypatch.setattr(Training, "LabelledWaves", lambda path: pytest.fail("the label file was read"))
    with pytest.raises(ValueError, match=message):
        Training.TrainFromWav(labelFile="absent.csv", seed=1, **kw)


NAMES = {"f2_gather_windows_mixed": 15, "f2_input_batch_smeared": 31, "f2_trainer_render_smeared": 15}


def test_the_entries_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    assert "Training at reduced resolution" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n in NAMES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(params) == len(args) == n, name
        for p, a in zip(params, args):
            if p.startswith("uint64_t "):
                assert a is ctypes.c_uint64, (name, p)
            elif p.startswith("uint32_t "):
                assert a is ctypes.c_uint32, (name, p)
            elif p.startswith("int "):
                assert a is ctypes.c_int, (name, p)
            elif p.startswith("double "):
                assert a is ctypes.c_double, (name, p)
            else:
                assert "*" in p and a is ctypes.c_void_p, (name, p)
        assert hasattr(_lib.Context, name[len("f2_"):])
    # f2_input_batch_smeared is f2_input_batch_coloured's list with mix, Km, mix_of behind seed; the render likewise
    col, sm = _lib.SIGNATURES["f2_input_batch_coloured"][1], _lib.SIGNATURES["f2_input_batch_smeared"][1]
    assert sm[:26] == col[:26] and sm[29:] == col[26:]
    col, sm = _lib.SIGNATURES["f2_trainer_render_coloured"][1], _lib.SIGNATURES["f2_trainer_render_smeared"][1]
    assert sm[:12] == col and len(sm) == 15
    lib = ctypes.CDLL(build.build_library())
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() == 115
    import inspect
    from f2cnn_amd.trainer import Trainer
    for fn in (Trainer.render, Trainer.render_wet):
        p = inspect.signature(fn).parameters
        assert p["mixes"].default is None and p["mix_of"].default is None
    sig = inspect.signature(Training.TrainFromWav).parameters
    assert sig["spreads"].default == () and sig["bands"].default == ()
