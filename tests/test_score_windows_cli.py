"""`cnn test`: the parts that need no GPU - the command line, the messages for missing files, the grouping of the label CSV's
rows, and f2_cnn_score_windows declared, exported and bound (library version 111)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, build, cli
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.scripts.CNN import Training


def test_parser_takes_the_command():
    a = cli.build_parser().parse_args(["cnn", "test", "--by", "phoneme", "--rows", "all"])
    assert a.cnn_command == "test" and a.by == "phoneme" and a.rows == "all"
    a = cli.build_parser().parse_args(["cnn", "test", "-i", "x.npy", "-l", "y.csv", "-m", "w.npz"])
    assert (a.inputFile, a.labelFile, a.model) == ("x.npy", "y.csv", "w.npz")
    assert "by" not in vars(a) and "rows" not in vars(a)                     # absent unless given: the other commands parse as before
    assert "test" in cli.CNN and "cnn test" in cli.__doc__ and "--by" in cli.__doc__ and "--rows" in cli.__doc__


@pytest.mark.parametrize("option,value", [("--by", "nonsense"), ("--rows", "some")])
def test_parser_refuses_another_value(option, value, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "test", option, value])
    assert e.value.code == 2
    assert option in capsys.readouterr().err


def test_missing_files_give_the_messages_of_cnn_train(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert cli.main(["cnn", "test"]) == 1
    assert "Please first generate the input data file with 'prepare input'" in capsys.readouterr().out
    np.save(tmp_path / "x.npy", np.ones((1, 11, 40), np.float32))
    assert cli.main(["cnn", "test", "--input", str(tmp_path / "x.npy")]) == 1
    assert "Please first generate a label data file with 'prepare label'" in capsys.readouterr().out
    assert cli.main(["cnn", "train"]) == 1                                    # the same words as `cnn train`
    assert "Please first generate the input data file with 'prepare input'" in capsys.readouterr().out


ROWS = [  # set, region, speaker, sentence, phoneme, timepoint, slope, p, sign
    ["TEST", "DR2", "MABC0", "SX1", "iy", "800", "0.5", "0.01", "1"],
    ["TRAIN", "DR1", "FXYZ0", "SI2", "aa", "960", "-0.2", "0.02", "0"],
    ["TEST", "DR1", "MABC0", "SX1", "aa", "1120", "0.1", "0.03", "1"],
    ["TRAIN", "DR2", "FQRS0", "SA1", "w", "1280", "-0.7", "0.01", "0"],
    ["TRAIN", "DR1", "FXYZ0", "SI2", "iy", "1440", "0.3", "0.04", "1"],
    ["TEST", "DR2", "MDEF0", "SX9", "aa", "1600", "-0.1", "0.02", "0"],
]


def test_grouping_of_the_label_rows():
    idx, signs, gid, names = Training.GroupLabelRows(ROWS, "phoneme", "all")
    assert idx.tolist() == [0, 1, 2, 3, 4, 5] and idx.dtype == np.int64
    assert signs.tolist() == [1, 0, 1, 0, 1, 0] and signs.dtype == np.uint8
    assert names == ["aa", "iy", "w"] and gid.tolist() == [1, 0, 0, 2, 1, 0] and gid.dtype == np.int32
    idx, signs, gid, names = Training.GroupLabelRows(ROWS, "phoneme", "test")
    assert idx.tolist() == [0, 2, 5] and signs.tolist() == [1, 1, 0]
    assert names == ["aa", "iy"] and gid.tolist() == [1, 0, 0]               # 'w' does not occur among the TEST rows
    idx, signs, gid, names = Training.GroupLabelRows(ROWS, "region", "train")
    assert idx.tolist() == [1, 3, 4] and names == ["DR1", "DR2"] and gid.tolist() == [0, 1, 0]
    idx, signs, gid, names = Training.GroupLabelRows(ROWS, "speaker", "all")
    assert names == ["FQRS0", "FXYZ0", "MABC0", "MDEF0"] and gid.tolist() == [2, 1, 2, 0, 1, 3]
    idx, signs, gid, names = Training.GroupLabelRows(ROWS, "set", "all")
    assert names == ["TEST", "TRAIN"] and gid.tolist() == [0, 1, 0, 1, 1, 0]
    idx, signs, gid, names = Training.GroupLabelRows(ROWS, None, "test")
    assert names == ["all"] and gid.tolist() == [0, 0, 0]
    idx, signs, gid, names = Training.GroupLabelRows([r for r in ROWS if r[0] == "TRAIN"], "phoneme", "test")
    assert len(idx) == len(signs) == len(gid) == 0 and names == []


def test_grouping_refuses_what_it_cannot_tally():
    many = [["TEST", "DR1", "S%04d" % i, "SX1", "aa", str(160 * i), "0.1", "0.01", "1"] for i in range(1025)]
    with pytest.raises(ValueError, match="1025 distinct values.*1024"):
        Training.GroupLabelRows(many, "speaker", "test")
    idx, _, gid, names = Training.GroupLabelRows(many[:1024], "speaker", "test")
    assert len(names) == 1024 and gid.tolist() == list(range(1024))
    assert Training.GroupLabelRows(many, "phoneme", "test")[3] == ["aa"]
    with pytest.raises(ValueError):
        Training.GroupLabelRows(ROWS, "sentence", "all")
    with pytest.raises(ValueError):
        Training.GroupLabelRows(ROWS, "phoneme", "some")
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        Training.GroupLabelRows([ROWS[0][:8] + ["2"]], None, "all")


def test_where_the_result_is_written():
    assert Training.TestResultPath("last_trained_model") == "last_trained_model_test.json"
    assert Training.TestResultPath(os.path.join("runs", "weights.npz")) == os.path.join("runs", "weights_test.json")
    assert Training.TestResultPath("weights.npz.bak") == "weights.npz.bak_test.json"
    assert Training.TestResultPath(F2CNNModel.glorot(rows=11, channels=40)) is None     # an object: nothing is written


def test_the_documents_quote_the_measured_numbers():
    """The timing table of DESIGN.md and the README bullet were written around placeholders (@NAME@) that a script fills from
    profiles/r13_score_windows_timing.json: none may be left, and the numbers quoted are the file's."""
    import glob
    import json
    docs = glob.glob(os.path.join(ROOT, "*.md")) + glob.glob(os.path.join(ROOT, "*", "README.md"))
    assert len(docs) >= 5
    for path in docs:
        left = re.findall(r"@[A-Z]+@", open(path).read())
        assert not left, (path, left)
    t = json.load(open(os.path.join(ROOT, "profiles", "r13_score_windows_timing.json")))
    new, old = "%.1f" % t["score_windows_ms"]["mean"], "%.1f" % t["parent_route_ms"]["mean"]
    design, readme = open(os.path.join(ROOT, "DESIGN.md")).read(), open(os.path.join(ROOT, "README.md")).read()
    section = design[design.index("### Scoring labelled windows"):]
    section = section[:section.index("\n### ", 10)]
    assert new in section and old in section and "%.1f" % t["ratio_parent_over_score_windows"] in section
    assert "{} ms against".format(new) in " ".join(readme.split()) and "{} ms for the route".format(old) in " ".join(readme.split())


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+f2_cnn_score_windows\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_cnn_score_windows is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["f2_ctx* ctx", "const f2_cnn* cnn", "const float* windows", "int64_t n", "int normalize", "const uint8_t* signs",
                      "const int32_t* groups_or_null", "int G", "float* scores_or_null", "uint8_t* labels_or_null", "int64_t* counts",
                      "double* loss_sum", "int mem_space"]
    res, args = _lib.SIGNATURES["f2_cnn_score_windows"]
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert res is i and args == [vp, vp, vp, ctypes.c_int64, i, vp, vp, i, vp, vp, vp, vp, i]
    assert list(inspect.signature(_lib.Context.cnn_score_windows).parameters)[1:11] == [
        "handle", "windows", "n", "normalize", "signs", "groups", "n_groups", "scores", "labels", "mem_space"]
    assert list(inspect.signature(F2CNNModel.evaluate).parameters)[1:] == ["x", "y", "groups", "n_groups", "normalize", "ctx"]
    assert list(inspect.signature(Training.TestModel).parameters)[:5] == ["labelFile", "inputFile", "model", "by", "rows"]
    lib = ctypes.CDLL(build.build_library())
    assert hasattr(lib, "f2_cnn_score_windows")
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() >= 111
