"""`--accuracy` on the evaluation commands: the parts that need no GPU - the command line takes the switch on the four
commands and parses as before without it, f2_label_accuracy is declared, exported and bound, the library says version 110 -
and the referee of tests/test_gpu_label_accuracy.py (tests/label_referee.py) held against its hand-worked cases."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import label_referee as lr
from conftest import ROOT
from f2cnn_amd import _lib, build, cli

COMMANDS = ("eval", "evalnoise", "evalrand", "noisesweep")


@pytest.mark.parametrize("command", COMMANDS)
def test_parser_takes_the_switch(command):
    parse = cli.build_parser().parse_args
    base = ["cnn", command, "--file", "a.WAV"]
    assert parse(base + ["--accuracy"]).accuracy == "reference"            # the bare flag
    assert parse(base + ["--accuracy", "centre"]).accuracy == "centre"
    assert parse(base + ["--accuracy", "reference"]).accuracy == "reference"
    assert parse(["cnn", command, "--accuracy", "--file", "a.WAV"]).file == "a.WAV"
    assert "accuracy" not in vars(parse(base))                              # without it the command parses as before
    assert "--accuracy" in cli.__doc__


@pytest.mark.parametrize("command", COMMANDS)
def test_parser_refuses_another_mode(command, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", command, "--file", "a.WAV", "--accuracy", "nearest"])
    assert e.value.code == 2
    assert "--accuracy" in capsys.readouterr().err


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+f2_label_accuracy\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_label_accuracy is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["f2_ctx* ctx", "const uint8_t* labels", "const int64_t* window_offsets", "int U", "const int64_t* ref_offsets",
                      "const int64_t* ref_timepoints", "const uint8_t* ref_signs", "int R", "int64_t origin", "int hop", "int step",
                      "int64_t* counts", "int mem_space"]
    res, args = _lib.SIGNATURES["f2_label_accuracy"]
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert res is i and args == [vp, vp, vp, i, vp, vp, vp, i, ctypes.c_int64, i, i, vp, i]
    assert list(inspect.signature(_lib.Context.label_accuracy).parameters)[1:10] == [
        "labels", "window_offsets", "ref_offsets", "ref_timepoints", "ref_signs", "origin", "hop", "step", "mem_space"]
    lib = ctypes.CDLL(build.build_library())
    assert hasattr(lib, "f2_label_accuracy")
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() >= 110


def test_evaluation_functions_take_the_keyword():
    from f2cnn_amd.scripts.CNN import Evaluating
    for fn in (Evaluating.EvaluateOneWavFile, Evaluating.EvaluateWithNoise, Evaluating.EvaluateRandom, Evaluating.EvaluateNoiseSweep):
        assert inspect.signature(fn).parameters["accuracy"].default is None, fn.__name__
    with pytest.raises(ValueError):
        Evaluating.EvaluateNoiseSweep([], [0.0], accuracy="nearest")


def test_reference_labels_without_side_files(tmp_path, monkeypatch):
    import f2cnn_oracle as orc
    from f2cnn_amd import wavio
    from f2cnn_amd.scripts.CNN import Evaluating
    monkeypatch.chdir(tmp_path)                       # (no configF2CNN.conf here: the configuration's defaults)
    wav = str(tmp_path / "DR1.NOFB0.SA2.WAV")
    wavio.write_sphere(wav, 16000, orc.synth_utterance(3, 8000))
    assert Evaluating.ReferenceLabels(wav) is None
    wav = lr.write_labelled_file(tmp_path, lambda n: orc.synth_utterance(5, n))
    t, s = Evaluating.ReferenceLabels(wav)
    assert t.dtype == np.int64 and s.dtype == np.uint8 and len(t) == len(s) >= 20
    assert (np.diff(t) > 0).all() and set(s.tolist()) == {0, 1}
    assert (t % 160 == 0).all() and t[0] >= 800       # one label per 10 ms step, the first a radius in


def test_referee_hand_worked_cases():
    lr.check_hand_cases()


@pytest.mark.parametrize("hop,origin", lr.CASES)
def test_referee_forms_agree_on_the_short_utterances(hop, origin):
    """the row loop handed to NumPy against the word-for-word double loop, on the utterances of a few hundred rows"""
    labels, wo, ro, T, s = lr.ragged_batch(hop, origin)
    for u in range(5):
        args = (labels[wo[u]:wo[u + 1]], T[ro[u]:ro[u + 1]], s[ro[u]:ro[u + 1]], origin, hop)
        assert np.array_equal(lr.referee(*args), lr.referee_loops(*args)), u
