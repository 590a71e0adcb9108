"""The host side of `cnn eval --segments` (no GPU): the penalty of a dwell time, the fixed-point pair the device takes, the two
tables, the command line, the tile constants against the header - and the condition the GPU tests' random streams must meet
(tests/segments_cases.py), asserted here where it can never be skipped."""
import math
import os
import re

import numpy as np
import pytest

import segments_cases as sc
import segments_referee as ref
from conftest import ROOT
from f2cnn_amd import _lib, cli, segments


def test_switch_penalty_is_the_log_odds_of_leaving():
    assert segments.SwitchPenalty(30.0, 160, 16000) == pytest.approx(math.log(2.0))          # a = 160 / 480
    assert segments.SwitchPenalty(30.0, 1, 16000) == pytest.approx(math.log(479.0))
    assert segments.SwitchPenalty(30.0, 240, 16000) == 0.0 and segments.SwitchPenalty(30.0, 4000, 16000) == 0.0   # a capped at 0.5
    assert segments.SwitchPenalty(60.0, 160, 16000) > segments.SwitchPenalty(30.0, 160, 16000)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            segments.SwitchPenalty(bad, 160, 16000)


def test_quantise_is_two_to_the_sixteen_per_nat():
    assert segments.EmissionWeight(160, 160) == 1.0 and segments.EmissionWeight(1, 160) == 1.0 / 160 and segments.EmissionWeight(400, 160) == 1.0
    assert segments.DefaultDwellMs(160, 16000) == 30.0
    scale, penalty = segments.Quantise(160, 160, 16000)
    assert scale == 65536.0 and penalty == round(65536 * math.log(2.0)) and isinstance(penalty, int)
    scale, penalty = segments.Quantise(16, 160, 16000, dwell_ms=50.0)
    assert scale == 6553.6 and penalty == round(65536 * math.log(49.0))
    assert segments.Quantise(16, 160, 16000, weight=0.5)[0] == 32768.0
    assert segments.Quantise(1, 160, 16000, dwell_ms=1e9)[1] <= _lib.PATH_MAX_PENALTY and 16 * 65536.0 <= _lib.PATH_MAX_SCALE
    with pytest.raises(ValueError):
        segments.Quantise(16, 160, 16000, weight=0.0)


def test_tile_constants_equal_the_header():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    assert int(re.search(r"#define F2_PATH_TILE (\d+)", text).group(1)) == _lib.PATH_TILE
    assert int(re.search(r"#define F2_PATH_SCAN_CHUNK (\d+)", text).group(1)) == _lib.PATH_SCAN_CHUNK
    for name in ("f2_decision_path", "f2_decision_runs", "f2_interval_tally", "f2_eval_segments_batch"):
        assert name in _lib.SIGNATURES
    # the fused call is the strided call up to `hop`, with the strided call's outputs first among its own
    base = _lib.SIGNATURES["f2_eval_batch_strided"][1]
    assert _lib.SIGNATURES["f2_eval_segments_batch"][1][:14] == base[:14]


def test_the_random_streams_stand_clear_of_half_integers():
    assert sc.clearance(sc.random_scores()) >= sc.CLEAR
    scores, wo, names = sc.adversarial()
    l = 65536.0 * ref.logits(scores)
    away = np.abs(l % 1.0 - 0.5)
    assert away[l != 0].min() >= sc.CLEAR and len(names) == len(wo) - 1


def test_phoneme_intervals_are_ordered_and_half_open():
    names, bounds = segments.PhonemeIntervals([("h#", 0, 100), ("ay", 100, 300), ("t", 290, 400), ("bad", 9, 3)])
    assert names == ["h#", "ay", "t"] and bounds.tolist() == [[0, 100], [100, 290], [290, 400]]
    assert segments.PhonemeIntervals(None)[1].shape == (0, 2)


def test_tables_hold_what_they_say():
    runs = np.array([[0, 3, 1, 3 * 65536], [3, 2, 0, -65536]], np.int64)
    lines = segments.RunsTable("X.WAV", runs, 800, 160, 16000, 65536.0, ["h#", "ay"], np.array([[0, 1000], [1000, 2000]]))
    assert "2 runs" in lines[0] and lines[1].split("\t")[2:] == ["start ms", "end ms", "duration ms", "decision", "mean log-odds", "phonemes"]
    first, second = (line.split("\t")[2:] for line in lines[2:])
    assert first == ["50.0", "70.0", "30.0", "rising", "+1.000", "h# ay"]          # rows at 800, 960, 1120
    assert second == ["80.0", "90.0", "20.0", "falling", "-0.500", "ay"]
    assert segments.RunsTable("X", runs, 800, 160, 16000, 65536.0)[2].split("\t")[-1] == ""
    tally = np.array([[4, 1, 0, -2 * 65536], [6, 3, 6, 3 * 65536], [0, 0, 0, 0], [4, 3, 4, 65536]], np.int64)
    order, rows = segments.CombinePhonemeTally(["h#", "ay", "q", "h#"], tally)
    assert order == ["h#", "ay", "q"] and rows.tolist() == [[8, 4, 4, -65536], [6, 3, 6, 3 * 65536], [0, 0, 0, 0]]
    table = [line.split("\t")[2:] for line in segments.PhonemeTable("X", ["h#", "ay", "q", "h#"], tally, 65536.0)]
    assert table[1] == ["phoneme", "rows", "% rising raw", "% rising smoothed", "mean log-odds"]
    assert table[2:] == [["h#", "8", "50.0", "50.0", "-0.125"], ["ay", "6", "50.0", "100.0", "+0.500"], ["q", "0", "-", "-", "-"]]


def test_command_line_takes_the_new_flags(capsys):
    p = cli.build_parser()
    a = p.parse_args(["cnn", "eval", "-f", "X.WAV", "--segments", "--dwell", "45", "--segments-weight", "0.25", "--hop", "frame"])
    assert a.segments is True and a.dwell == 45.0 and a.segments_weight == 0.25
    assert p.parse_args(["cnn", "evalrand", "--segments", "--segments-weight", "auto"]).segments_weight == "auto"
    assert "segments" not in p.parse_args(["cnn", "eval", "-f", "X.WAV"])
    for bad in ("0", "-1", "17", "heavy"):
        with pytest.raises(SystemExit):
            p.parse_args(["cnn", "eval", "-f", "X.WAV", "--segments", "--segments-weight", bad])
    capsys.readouterr()
    assert cli.main(["cnn", "eval", "-f", "X.WAV", "--dwell", "45"]) == 1 and "belong to --segments" in capsys.readouterr().out
    assert cli.main(["cnn", "eval", "-f", "X.WAV", "--segments", "--dwell", "0"]) == 1
    assert cli.main(["cnn", "noisesweep", "-f", "X.WAV", "--snrs", "0", "--segments"]) == 1 and "--segments is not supported" in capsys.readouterr().out
