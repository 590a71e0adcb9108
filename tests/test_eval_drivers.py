"""`cnn eval`, `evalnoise` and `evalrand` held against a stub context that stands in for the device (tests/eval_stub.py): which
device calls each command makes for each set of options, which keys its .F2CNN.npz holds, that `evalrand` writes and prints for a
file what `eval` writes and prints for it - the corpus has a file of another rate, so every group of `evalrand` is a mixed one and
goes file by file - and that two maps in one run are refused before the model is read. `resample=` needs the device
(tests/test_gpu_resample.py)."""
import collections
import os

import numpy as np
import pytest

import eval_stub
from eval_stub import MATRIX, OPTION_SETS, WIDTH
from f2cnn_amd import _lib

RADIUS = 5
I16, F64 = _lib.WAVE_I16, _lib.WAVE_F64
# file -> (samples, rate, intervals of its .PHN, has .FB / .PHN labels); the order of eval_stub.build_corpus
FILES = [(19200, 16000, 4, True), (4000, 16000, 0, False), (2000, 8000, 0, False)]
PATCHES = 16                                      # 128 channels in bands of 8

# (a) the device calls of one file's pass, per option set; a name that is no Context method stands for the plain evaluation
PASS_CALLS = {
    "none": ["plain"],
    "figure": ["eval_figure_batch"],
    "occlusion": ["eval_occlusion_batch"],
    "occlusion+figure": ["eval_occlusion_batch", "score_track"],
    "saliency": ["eval_saliency_batch"],
    "saliency+figure": ["eval_saliency_batch", "score_track"],
    "segments": ["eval_segments_batch"],
    "segments+figure": ["eval_figure_batch", "decision_path", "decision_runs", "interval_tally"],
    "segments+occlusion": ["eval_occlusion_batch", "decision_path", "decision_runs", "interval_tally"],
    "segments+saliency+figure": ["eval_saliency_batch", "score_track", "decision_path", "decision_runs", "interval_tally"],
}
# (b) the keys an option adds to a file's .npz, in the order `cnn eval` stores them
KEYS = {
    "hop": ["hop", "timepoints"],
    "accuracy": ["accuracy", "confusion", "accuracy_mode"],                         # (a file with .FB / .PHN)
    "figure": ["figure_track", "figure_span"],
    "occlusion": ["occlusion_" + k for k in ("patches", "fill", "scores", "summary", "map", "span", "hz")],
    "saliency": ["saliency_map", "saliency_summary", "saliency_span"],
    "smoothed accuracy": ["segments_accuracy", "segments_confusion"],               # (segments and accuracy, such a file)
    "segments": ["segments_" + k for k in ("path", "runs", "run_offsets", "value", "logit_scale", "penalty", "hop")],
    "phonemes": ["segments_phoneme_names", "segments_phoneme_tally"],               # (segments, a file with a .PHN)
}


def rows_of(samples, rate, hop):
    step = rate // 100
    return samples - (2 * RADIUS + 1) * step if hop is None else _lib.strided_window_count(samples, RADIUS, step, hop)


def pass_log(index, name, hop, dtype):
    """the log of one file's pass: B = 1, the file's samples, the hop the device sees"""
    samples, rate, intervals, _ = FILES[index]
    step, device_hop, rows = rate // 100, 1 if hop is None else hop, [rows_of(samples, rate, hop)]
    log = []
    for method in PASS_CALLS[name]:
        if method == "plain":
            log.append(("eval_utterance" if hop is None else "eval_batch_strided", 1, [samples], dtype, hop, step, False, 0.0, None, None))
        elif method.startswith("eval_"):
            K = {"eval_occlusion_batch": PATCHES, "eval_segments_batch": intervals}.get(method)
            log.append((method, 1, [samples], dtype, device_hop, step, False, 0.0, None if method == "eval_segments_batch" else WIDTH, K))
        elif method == "score_track":
            log.append((method, 1, rows, None, device_hop, None, None, None, WIDTH, None))
        elif method == "interval_tally":
            log.append((method, 1, rows, None, device_hop, None, None, None, None, intervals))
        else:
            log.append((method, 1, rows, None, None, None, None, None, None, None))
    return log


def accuracy_log(index, name, accuracy, hop):
    """[the f2_label_accuracy call of a file's decisions, that of its smoothed decisions]: those of them the run makes"""
    samples, rate, _, labelled = FILES[index]
    if accuracy is None or not labelled:
        return []
    one = ("label_accuracy", 1, [rows_of(samples, rate, hop)], None, 1 if hop is None else hop, rate // 100, None, None, None, 1)
    return [one] * (2 if "segments" in OPTION_SETS[name] else 1)


def expected_keys(index, name, accuracy, hop):
    labelled, options = FILES[index][3], OPTION_SETS[name]
    keys = ["scores", "labels"] + (KEYS["hop"] if hop is not None else []) + (KEYS["accuracy"] if accuracy and labelled else [])
    for option in ("figure", "occlusion", "saliency"):
        keys += KEYS[option] if option in options else []
    if "segments" in options:
        keys += (KEYS["smoothed accuracy"] if accuracy and labelled else []) + KEYS["segments"] + (KEYS["phonemes"] if labelled else [])
    return keys


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp("evaldrivers")
    return root, eval_stub.build_corpus(root)


_runs = {}


def runs(corpus, command, case):
    """the calls of `command` for the case, run once"""
    if (command, case) not in _runs:
        name, accuracy, hop = case
        _runs[command, case] = eval_stub.run_command(corpus[0], command, OPTION_SETS[name], accuracy, hop, corpus[1])
        assert all(call["error"] is None for call in _runs[command, case]), [call["error"] for call in _runs[command, case]]
        assert command != "eval" or all(call["returned"] == 0 for call in _runs[command, case])
    return _runs[command, case]


def of_file(calls, path):
    """{key: array} of the one .npz a run wrote for the file"""
    stem = os.path.splitext(os.path.basename(path))[0]
    found = [members for call in calls for written, members in call["npz"].items() if os.path.basename(written).startswith(stem)]
    assert len(found) == 1, (path, [list(call["npz"]) for call in calls])
    return found[0]


CASES = pytest.mark.parametrize("case", MATRIX, ids=["{}-{}-hop{}".format(*case) for case in MATRIX])


@CASES
def test_device_calls(corpus, case):
    name, accuracy, hop = case
    files = corpus[1]
    for command, dtype in (("eval", I16), ("evalnoise", F64)):
        for index, call in enumerate(runs(corpus, command, case)):
            assert call["log"] == pass_log(index, name, hop, dtype) + accuracy_log(index, name, accuracy, hop), (command, files[index])
    call, = runs(corpus, "evalrand", case)
    order = [files.index(f) for f in call["files"]]
    assert sorted(order) == [0, 1, 2]
    # a mixed group: one pass per file, B = 1, in the order of the files; then the group's accuracy pass; then, in the files' tails,
    # the accuracy of the smoothed decisions
    want = [entry for index in order for entry in pass_log(index, name, hop, I16)]
    assert call["log"] == want + [entry for index in order for entry in accuracy_log(index, name, accuracy, hop)]
    if name == "none":
        assert [entry[:2] for entry in call["log"][:3]] == [("eval_utterance" if hop is None else "eval_batch_strided", 1)] * 3


@CASES
def test_npz_keys(corpus, case):
    name, accuracy, hop = case
    for index, path in enumerate(corpus[1]):
        want = expected_keys(index, name, accuracy, hop)
        assert list(of_file(runs(corpus, "eval", case), path)) == want, path
        assert list(of_file(runs(corpus, "evalnoise", case), path)) == want, path
        # (evalrand may store a file's blocks in another order: compared as sets)
        assert sorted(of_file(runs(corpus, "evalrand", case), path)) == sorted(want), path


@CASES
def test_evalrand_writes_what_eval_writes(corpus, case):
    for path in corpus[1]:
        alone, grouped = of_file(runs(corpus, "eval", case), path), of_file(runs(corpus, "evalrand", case), path)
        assert set(alone) == set(grouped)
        for key, value in alone.items():
            got = grouped[key]
            assert got.dtype == value.dtype and got.shape == value.shape and got.tobytes() == value.tobytes(), (path, key)
    # the pictures too
    pictures = {p: data for call in runs(corpus, "eval", case) for p, data in call["png"].items()}
    assert runs(corpus, "evalrand", case)[0]["png"] == pictures
    assert len(pictures) == 3 * sum(option in OPTION_SETS[case[0]] for option in ("figure", "occlusion", "saliency"))


@CASES
def test_evalrand_prints_what_eval_prints(corpus, case):
    """the lines of evalrand up to its corpus summary, less its header, are those of the three eval runs, less theirs - as a multiset:
    evalrand prints a group's accuracy lines before the files' blocks"""
    alone = collections.Counter()
    for call in runs(corpus, "eval", case):
        lines = call["stdout"].splitlines()
        assert lines[0].startswith("Using model") and lines[1].startswith("File:")
        alone.update(lines[2:])
    lines = runs(corpus, "evalrand", case)[0]["stdout"].splitlines()
    end = lines.index("Evaluating network on all files.")
    assert lines[0] == "" and lines[1].startswith("####") and lines[2].startswith("Evaluating network on 3 WAV files")
    assert collections.Counter(lines[3:end]) == alone
    assert sum("done !" in line for line in lines) == 3


@pytest.mark.parametrize("command", eval_stub.COMMANDS)
def test_two_maps_are_refused_before_the_model_is_read(corpus, command):
    from f2cnn_amd.model import F2CNNModel
    # (evalrand loads its model before the first file: it gets a real one)
    model = F2CNNModel.glorot(7) if command == "evalrand" else object()
    options = dict(occlusion=True, saliency=True)
    if command == "eval":                          # (through its function: the command line refuses the pair itself)
        from f2cnn_amd.scripts.CNN import Evaluating
        call = eval_stub.run_function(corpus[0], lambda: Evaluating.EvaluateOneWavFile(corpus[1][0], model=model, hop=160, **options))
    else:
        call = eval_stub.run_command(corpus[0], command, options, None, 160, corpus[1][:1], model=model)[0]
    assert call["error"] == ("ValueError", "one map per pass: occlusion= or saliency=, not both")
    assert call["log"] == [] and call["npz"] == {} and call["png"] == {}
