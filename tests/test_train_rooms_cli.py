"""`cnn train --engine hip --from-wav --augment-t60 / --augment-rirs`: what the command line refuses and hands on, the epoch's room
draw, and the declarations of the three entries. No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, cli, reverb
from f2cnn_amd.scripts.CNN import Training

REFUSALS = [(["cnn", "train", "--engine", "hip", "--augment-t60", "0.2"], "--augment-t60 needs --from-wav"),
            (["cnn", "train", "--engine", "hip", "--augment-rirs", "a.wav"], "--augment-rirs needs --from-wav"),
            (["cnn", "train", "--from-wav", "--augment-t60", "0.2"], "--from-wav needs --engine hip"),
            (["cnn", "train", "--augment-t60", "0.2"], "--augment-t60 needs --engine hip"),
            (["cnn", "train", "--engine", "torch", "--augment-t60", "0.2"], "--augment-t60 needs --engine hip"),
            (["cnn", "train", "--engine", "torch", "--from-wav", "--augment-rirs", "a.wav"], "--from-wav needs --engine hip"),
            (["cnn", "eval", "--file", "a.WAV", "--augment-t60", "0.2"], "--augment-t60 only applies to 'cnn train'"),
            # the messages of the flags that were there stay as they were, rooms or not
            (["cnn", "train", "--engine", "hip", "--augment-snrs", "20", "--augment-t60", "0.2"],
             "--augment-snrs needs --from-wav: stored windows cannot be rendered again under noise")]


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


@pytest.mark.parametrize("flag,text", [("--augment-t60", "0.2,abc"), ("--augment-t60", "0.2,-1"), ("--augment-t60", ""), ("--augment-t60", "inf"),
                                       ("--augment-rirs", "a.wav,,b.wav")])
def test_a_bad_list_is_a_usage_error(flag, text, capsys):
    with pytest.raises(SystemExit) as ei:
        cli.main(["cnn", "train", "--engine", "hip", "--from-wav", flag, text])
    assert ei.value.code == 2 and flag + " takes a comma-separated list" in capsys.readouterr().err


def test_main_hands_the_rooms_to_TrainFromWav(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    called = []
    monkeypatch.setattr(Training, "TrainFromWav", lambda **kw: called.append(kw))
    open("mine.csv", "w").close()
    base = ["cnn", "train", "--engine", "hip", "--from-wav", "-l", "mine.csv"]
    assert cli.main(base + ["--augment-t60", "0.2,0.4,0.8", "--seed", "9"]) == 0
    assert called.pop() == dict(labelFile="mine.csv", LPF=False, CUTOFF=None, snrs=(), seed=9, t60s=(0.2, 0.4, 0.8), rirs=(), drr_db=0.0)
    assert cli.main(base + ["--augment-rirs", "a.wav,b.wav", "--augment-t60", "0.3", "--drr", "-3", "--augment-snrs", "20,3", "--lpf", "50"]) == 0
    assert called.pop() == dict(labelFile="mine.csv", LPF=True, CUTOFF=50, snrs=(20.0, 3.0), seed=None, t60s=(0.3,), rirs=("a.wav", "b.wav"),
                                drr_db=-3.0)
    assert cli.main(base + ["--augment-snrs", "20"]) == 0                     # without rooms: the call it was
    assert called.pop() == dict(labelFile="mine.csv", LPF=False, CUTOFF=None, snrs=(20.0,), seed=None)


def test_the_room_draw_is_the_seeds_and_leaves_the_noise_draw_alone():
    assert Training.ROOM_STREAM != Training.NOISE_STREAM and Training.VALIDATION_ROOM_SEED != Training.VALIDATION_NOISE_SEED
    draws = []
    for _ in range(2):
        rng = np.random.default_rng([5, Training.ROOM_STREAM])
        draws.append([Training.draw_epoch_rooms(rng, 3, 40) for _ in range(3)])
    for (r0, s0), (r1, s1) in zip(*draws):
        assert np.array_equal(r0, r1) and s0 == s1 and r0.dtype == np.int32 and r0.shape == (40,)
    rooms = np.concatenate([r for r, _ in draws[0]])
    assert set(rooms.tolist()) == {0, 1, 2, 3} and len({s for _, s in draws[0]}) == 3                 # 3 is the dry one
    other = Training.draw_epoch_rooms(np.random.default_rng([6, Training.ROOM_STREAM]), 3, 40)
    assert not np.array_equal(other[0], draws[0][0][0]) and other[1] != draws[0][0][1]
    # the noise generator is one of its own: drawing rooms in between does not move it
    a = np.random.default_rng([5, Training.NOISE_STREAM])
    b = np.random.default_rng([5, Training.NOISE_STREAM])
    room_rng = np.random.default_rng([5, Training.ROOM_STREAM])
    for _ in range(3):
        la, sa = Training.draw_epoch_noise(a, 2, 40)
        Training.draw_epoch_rooms(room_rng, 3, 40)
        lb, sb = Training.draw_epoch_noise(b, 2, 40)
        assert np.array_equal(la, lb) and sa == sb
    assert not np.array_equal(Training.draw_epoch_noise(np.random.default_rng([5, Training.NOISE_STREAM]), 3, 40)[0], draws[0][0][0])


def test_build_rooms():
    measured = [np.array([1.0, 0.5])]
    hs = Training.build_rooms((0.01, 0.02), measured, 16000, -3.0, 77)
    assert [len(h) for h in hs] == [160, 320, 2] and hs[2] is measured[0]
    for level, (h, t60) in enumerate(zip(hs, (0.01, 0.02))):
        assert np.array_equal(h, reverb.SyntheticRIR(t60, 16000, -3.0, 77, level))
    assert not np.array_equal(hs[0], Training.build_rooms((0.01,), (), 16000, -3.0, 78)[0])


def test_a_room_beyond_the_longest_response_is_refused_before_any_device_work(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(_lib, "default_context", lambda *a, **k: pytest.fail("the device was opened"))
    with pytest.raises(ValueError, match="at most {}".format(reverb.MAX_TAPS)):
        Training.TrainFromWav(labelFile="absent.csv", t60s=(0.2, 2.5), seed=1)


def test_the_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n in {"f2_reverb_pick": 11, "f2_input_batch_wet": 26, "f2_trainer_render_wet": 10}.items():
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
    # f2_input_batch_wet is f2_input_batch_noisy's list with the four room arguments in front of the noise arguments
    noisy, wet = _lib.SIGNATURES["f2_input_batch_noisy"][1], _lib.SIGNATURES["f2_input_batch_wet"][1]
    assert wet[:16] == noisy[:16] and wet[20:] == noisy[16:]
    assert hasattr(__import__("f2cnn_amd.trainer", fromlist=["Trainer"]).Trainer, "render_wet")
