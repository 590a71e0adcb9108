"""`cnn noisesweep`: the parts that need no GPU - the command line takes the new command and its options and leaves
`cnn evalnoise` as it was, the C entry point is declared, exported and bound, and the library says version 109."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT
from f2cnn_amd import _lib, build, cli


def test_parser_takes_the_sweep():
    args = cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "20,10,-3", "--seed", "5", "--hop", "frame"])
    assert args.cnn_command == "noisesweep" and args.file == "a.WAV"
    assert args.snrs == [20.0, 10.0, -3.0] and args.seed == 5 and args.hop == "frame" and args.save_wavs is False
    assert cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "0", "--save-wavs"]).save_wavs is True
    assert "noisesweep" in cli.CNN and "noisesweep" in cli.__doc__


@pytest.mark.parametrize("bad", ["20,x", "", "20,,10", "nan", "inf,3"])
def test_parser_refuses_a_malformed_list(bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "noisesweep", "--file", "a.WAV", "--snrs", bad])
    assert e.value.code == 2
    assert "--snrs" in capsys.readouterr().err


def test_evalnoise_parses_as_before():
    args = vars(cli.build_parser().parse_args(["cnn", "evalnoise", "--file", "a.WAV", "--noise", "-3"]))
    before = dict(configure=False, file="a.WAV", inputFile=None, labelFile=None, model=None, cnn_command="evalnoise", CUTOFF=None,
                  count=None, SNRdB=-3.0, hop=None)
    assert {k: args[k] for k in before} == before
    assert sorted(set(args) - set(before)) == ["save_wavs", "seed", "snrs"]
    assert args["snrs"] is None and args["seed"] is None and args["save_wavs"] is False


def test_sweep_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+f2_eval_noise_sweep\s*\(([^;]*)\)\s*;", code)
    assert m, "f2_eval_noise_sweep is not declared in include/f2cnn_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert len(params) == 24
    assert params[13:17] == ["int hop", "const double* snr_db", "int K", "uint64_t seed"]
    assert params[17:] == ["double* noisy_or_null", "float* scores_or_null", "uint8_t* labels_or_null", "int64_t* window_offsets_or_null",
                           "double* sigma_or_null", "int64_t* stats_or_null", "int mem_space"]
    for word in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "Evaluating.py:199"):
        assert word in text, word
    res, args = _lib.SIGNATURES["f2_eval_noise_sweep"]
    assert res is ctypes.c_int and len(args) == len(params)
    # the binding is f2_eval_batch_strided's up to `hop`, then the levels and the seed, then the outputs
    base = _lib.SIGNATURES["f2_eval_batch_strided"][1]
    assert args[:14] == base[:14] and args[14:17] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64]
    assert args[17:] == [ctypes.c_void_p] * 6 + [ctypes.c_int]
    p = inspect.signature(_lib.Context.eval_noise_sweep).parameters
    assert "snr_db" in p and "seed" in p and "hop" in p
    from f2cnn_amd.scripts.CNN import Evaluating
    p = inspect.signature(Evaluating.EvaluateNoiseSweep).parameters
    assert list(p)[:2] == ["files", "SNRdBs"]
    assert (p["seed"].default, p["hop"].default, p["LPF"].default, p["CUTOFF"].default, p["model"].default, p["save_wavs"].default) == \
        (0, None, False, 50, "last_trained_model", False)


def test_built_library_exports_the_sweep_and_says_109():
    lib = ctypes.CDLL(build.build_library())
    assert hasattr(lib, "f2_eval_noise_sweep")
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() >= 109
