"""`cnn train --engine hip --from-wav --augment-snrs ... --augment-colours / --augment-noise-taps`: what the command line refuses and
hands on, the level plan, the epoch's draw, the filters' errors before any file is read, and the declarations of the three entries.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, build, cli, noise
from f2cnn_amd.scripts.CNN import Evaluating, Training

TRAIN = ["cnn", "train", "--engine", "hip", "--from-wav"]
REFUSALS = [(TRAIN + ["--augment-colours", "pink"], "--augment-colours needs --augment-snrs"),
            (TRAIN + ["--augment-snrs", "20", "--augment-noise-taps", "255"], "--augment-noise-taps belongs to --augment-colours"),
            (TRAIN + ["--augment-noise-taps", "255"], "--augment-noise-taps belongs to --augment-colours"),
            (["cnn", "train", "--engine", "hip", "--augment-snrs", "20", "--augment-colours", "pink"], "--augment-snrs needs --from-wav"),
            (["cnn", "train", "--from-wav", "--augment-snrs", "20", "--augment-colours", "pink"], "--from-wav needs --engine hip"),
            (["cnn", "train", "--augment-colours", "pink"], "--augment-colours needs --augment-snrs"),
            (["cnn", "eval", "--file", "a.WAV", "--augment-colours", "pink"], "--augment-colours only applies to 'cnn train'"),
            (["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "20", "--augment-colours", "pink"], "--augment-colours only applies to 'cnn train'"),
            (["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "20", "--augment-noise-taps", "5"], "--augment-noise-taps only applies to 'cnn train'"),
            (TRAIN + ["--augment-snrs", ",".join(str(v) for v in range(13)), "--augment-colours", "white,pink,brown,speech,fir:a.npy"],
             "at most 64 noise levels, not 5 colours x 13 SNRs = 65"),
            # the sweep's own options stay refused on train
            (TRAIN + ["--augment-snrs", "20", "--colours", "pink"], "--colours only applies to 'cnn noisesweep'"),
            (TRAIN + ["--augment-snrs", "20", "--augment-colours", "pink", "--noise-taps", "255"], "--noise-taps only applies to 'cnn noisesweep'")]


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


@pytest.mark.parametrize("flag,text,word", [("--augment-colours", "pink,purple", "takes a comma-separated list"),
                                            ("--augment-colours", "", "takes a comma-separated list"),
                                            ("--augment-colours", "like:", "takes a comma-separated list"),
                                            ("--augment-noise-taps", "256", "takes an odd, positive number of taps"),
                                            ("--augment-noise-taps", "abc", "takes an odd, positive number of taps")])
def test_a_bad_value_is_a_usage_error(flag, text, word, capsys):
    with pytest.raises(SystemExit) as ei:
        cli.main(TRAIN + ["--augment-snrs", "20", flag, text])
    assert ei.value.code == 2 and flag + " " + word in capsys.readouterr().err


def test_parser_values():
    args = cli.build_parser().parse_args(TRAIN + ["--augment-snrs", "20,0", "--augment-colours", "pink,like:babble.wav,fir:t.npy",
                                                  "--augment-noise-taps", "255"])
    assert args.augment_colours == ["pink", "like:babble.wav", "fir:t.npy"] and args.augment_noise_taps == 255
    assert "colours" not in args and "noise_taps" not in args
    args = cli.build_parser().parse_args(TRAIN + ["--augment-snrs", "20"])
    assert "augment_colours" not in args and "augment_noise_taps" not in args
    assert "--augment-colours" in cli.__doc__ and "--augment-noise-taps" in cli.__doc__


def test_main_hands_the_colours_to_TrainFromWav(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    called = []
    monkeypatch.setattr(Training, "TrainFromWav", lambda **kw: called.append(kw))
    open("mine.csv", "w").close()
    base = TRAIN + ["-l", "mine.csv"]
    assert cli.main(base + ["--augment-snrs", "20,0", "--augment-colours", "pink,speech", "--seed", "9"]) == 0
    assert called.pop() == dict(labelFile="mine.csv", LPF=False, CUTOFF=None, snrs=(20.0, 0.0), seed=9, colours=("pink", "speech"))
    assert cli.main(base + ["--augment-snrs", "3", "--augment-colours", "white", "--augment-noise-taps", "255", "--augment-t60", "0.3", "--lpf", "50"]) == 0
    assert called.pop() == dict(labelFile="mine.csv", LPF=True, CUTOFF=50, snrs=(3.0,), seed=None, t60s=(0.3,), rirs=(), drr_db=0.0,
                                colours=("white",), noise_taps=255)
    assert cli.main(base + ["--augment-snrs", "20"]) == 0                     # without colours: the call it was
    assert called.pop() == dict(labelFile="mine.csv", LPF=False, CUTOFF=None, snrs=(20.0,), seed=None)


class Planned(Exception):
    pass


def test_the_level_plan_is_the_sweeps(tmp_path, monkeypatch):
    """TrainFromWav builds one filter per level of Evaluating.ColourLevels, colour-major over the SNRs, each colour once, before it
    looks for the label file"""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(_lib, "default_context", lambda *a, **k: pytest.fail("the device was opened"))
    built = []
    real = noise.FromSpec

    def from_spec(spec, framerate, taps=1025):
        built.append((spec, framerate, taps))
        return real(spec, framerate, taps)
    monkeypatch.setattr(noise, "FromSpec", from_spec)
    monkeypatch.setattr(Training, "LabelledWaves", lambda path: (_ for _ in ()).throw(Planned(path)))
    with pytest.raises(Planned):
        Training.TrainFromWav(labelFile="absent.csv", snrs=(20, 0), colours=("pink", "white", "pink"), noise_taps=255, seed=1)
    assert built == [("pink", 16000, 255), ("white", 16000, 255)]
    grid = Evaluating.ColourLevels(("pink", "speech"), (20.0, 0.0))
    assert [(c, v) for c, _, v in grid] == [("pink", 20.0), ("pink", 0.0), ("speech", 20.0), ("speech", 0.0)]
    # white is the unit filter, and its level numbers are the SNR numbers
    assert np.array_equal(noise.ColourFIR("white", 16000, 1025), [1.0])
    assert [v for _, _, v in Evaluating.ColourLevels(("white",), (20.0, 3.0))] == [20.0, 3.0]


def test_the_draw_of_an_epoch_is_unchanged():
    """draw_epoch_noise(rng, K, B): the levels first, then the seed - whatever K counts"""
    for K in (2, 6):
        a, b = np.random.default_rng([5, Training.NOISE_STREAM]), np.random.default_rng([5, Training.NOISE_STREAM])
        for _ in range(3):
            level_of, seed = Training.draw_epoch_noise(a, K, 40)
            want = b.integers(0, K + 1, 40).astype(np.int32)
            assert level_of.dtype == np.int32 and np.array_equal(level_of, want) and seed == int(b.integers(0, 2 ** 63))
            assert level_of.min() >= 0 and level_of.max() <= K
    levels = np.concatenate([Training.draw_epoch_noise(np.random.default_rng([5, Training.NOISE_STREAM]), 6, 400)[0]])
    assert set(levels.tolist()) == set(range(7))


@pytest.mark.parametrize("kw,message", [(dict(colours=("purple",)), "unknown noise colour"),
                                        (dict(colours=("pink",), noise_taps=4097), "at most {}".format(noise.MAX_TAPS)),
                                        (dict(colours=("pink",), noise_taps=256), "odd, positive number of taps"),
                                        (dict(colours=("pink",), snrs=()), "need the SNRs"),
                                        (dict(colours=("white", "pink", "brown", "speech", "fir:a.npy"), snrs=tuple(range(13))), "at most 64 levels")])
def test_filter_errors_come_before_any_file_is_read(kw, message, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(_lib, "default_context", lambda *a, **k: pytest.fail("the device was opened"))
    monkeypatch.setattr(Training, "LabelledWaves", lambda path: pytest.fail("the label file was read"))
    with pytest.raises(ValueError, match=message):
        Training.TrainFromWav(labelFile="absent.csv", seed=1, **dict(dict(snrs=(20.0,)), **kw))


def test_a_recording_at_another_rate_is_refused_before_any_file_is_read(tmp_path, monkeypatch):
    import wave
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(_lib, "default_context", lambda *a, **k: pytest.fail("the device was opened"))
    monkeypatch.setattr(Training, "LabelledWaves", lambda path: pytest.fail("the label file was read"))
    with wave.open("babble.wav", "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(8000)
        w.writeframes((np.random.default_rng(0).standard_normal(4000) * 1000).astype(np.int16).tobytes())
    with pytest.raises(ValueError, match="8000 Hz"):
        Training.TrainFromWav(labelFile="absent.csv", snrs=(20.0,), colours=("like:babble.wav",), seed=1)


NAMES = {"f2_shaped_noise_pick": 15, "f2_input_batch_coloured": 28, "f2_trainer_render_coloured": 12}


def test_the_entries_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    assert "Training against colours" in text
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
    # f2_input_batch_coloured is f2_input_batch_wet's list with fir, fir_offsets behind snr_db; the render likewise
    wet, col = _lib.SIGNATURES["f2_input_batch_wet"][1], _lib.SIGNATURES["f2_input_batch_coloured"][1]
    assert col[:20] == wet[:20] and col[22:] == wet[20:]
    wet, col = _lib.SIGNATURES["f2_trainer_render_wet"][1], _lib.SIGNATURES["f2_trainer_render_coloured"][1]
    assert col[:7] == wet[:7] and col[9:] == wet[7:]
    # the library exports them, and f2_version stays where it is: callers look the symbols up
    lib = ctypes.CDLL(build.build_library())
    for name in NAMES:
        assert hasattr(lib, name), name
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() == 115
    import inspect
    from f2cnn_amd.trainer import Trainer
    for fn in (Trainer.render, Trainer.render_wet):
        assert inspect.signature(fn).parameters["firs"].default is None
    sig = inspect.signature(Training.TrainFromWav).parameters
    assert sig["colours"].default == () and sig["noise_taps"].default == 1025
