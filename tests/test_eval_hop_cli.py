"""`cnn eval --hop`: the parts that need no GPU - the C entry point is declared, exported and bound, the command line takes
the flag, and the window count / timepoints the Python side sizes its arrays with are the ones the header states."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, build, cli

RADIUS, STEP = 5, 160
R = 2 * RADIUS + 1


def test_strided_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+f2_eval_batch_strided\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_eval_batch_strided is not declared in include/f2cnn_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 18
    assert params[13] == "int hop" and params[16].startswith("int64_t* window_offsets_or_null") and params[17] == "int mem_space"
    assert "Evaluating.py:71-87" in text
    lib = ctypes.CDLL(build.build_library())
    assert hasattr(lib, "f2_eval_batch_strided")
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() >= 108
    res, args = _lib.SIGNATURES["f2_eval_batch_strided"]
    assert res is ctypes.c_int and len(args) == len(params)
    # the binding is f2_eval_batch's with `hop` before the outputs and the window offsets behind them
    base = _lib.SIGNATURES["f2_eval_batch"][1]
    assert args == base[:13] + [ctypes.c_int] + base[13:15] + [ctypes.c_void_p] + base[15:]
    assert "hop" in inspect.signature(_lib.Context.eval_batch_strided).parameters


@pytest.mark.parametrize("command", ["eval", "evalnoise", "evalrand"])
def test_parser_takes_hop_on_the_three_commands(command, capsys):
    parser = cli.build_parser()
    assert parser.parse_args(["cnn", command, "--hop", "16"]).hop == 16
    assert parser.parse_args(["cnn", command, "--hop", "frame"]).hop == "frame"
    assert parser.parse_args(["cnn", command]).hop is None
    for bad in ("0", "-3", "1.5", "frames"):
        with pytest.raises(SystemExit):
            parser.parse_args(["cnn", command, "--hop", bad])
    assert "--hop" in capsys.readouterr().err


def test_python_entry_points_take_hop():
    from f2cnn_amd.scripts.CNN import Evaluating
    for name in ("EvaluateOneWavArray", "EvaluateWavArrays", "EvaluateOneWavFile", "EvaluateRandom", "EvaluateWithNoise"):
        p = inspect.signature(getattr(Evaluating, name)).parameters
        assert "hop" in p and p["hop"].default is None, name


# (n, hop): no windows (n <= 11 * step), exactly one, nb a multiple of hop and not, hop larger than nb
TABLE = [(0, 1), (1700, 16), (1760, 1), (1760, 160), (1761, 1), (1761, 160), (1762, 2), (1763, 2), (4000, 1), (4000, 3), (4000, 7),
         (4000, 16), (4000, 160), (4000, 161), (16000, 160), (16000, 100), (16000, 14240), (16000, 14241), (23456, 5)]


@pytest.mark.parametrize("n,hop", TABLE)
def test_window_count_and_timepoints(n, hop):
    nb = max(0, n - R * STEP)
    want = (nb + hop - 1) // hop                                  # ceil(nb / hop), the header's nbh_b
    assert want == len(range(0, nb, hop))                         # = the rows [::hop] keeps of nb every-sample rows
    assert _lib.strided_window_count(n, RADIUS, STEP, hop) == want
    tp = _lib.strided_timepoints(n, RADIUS, STEP, hop)
    assert tp.dtype == np.int64 and tp.shape == (want,)
    assert np.array_equal(tp, RADIUS * STEP + hop * np.arange(want))
    if want:
        # every window lies inside the utterance, and the next one would not be an every-sample window any more
        assert tp[-1] + RADIUS * STEP < n and tp[-1] - RADIUS * STEP + hop >= nb


def test_window_count_refuses_a_hop_below_one():
    for hop in (0, -1):
        with pytest.raises(ValueError):
            _lib.strided_window_count(4000, RADIUS, STEP, hop)
