"""Host side of `--resample` (no GPU): the filter design and the formula f2_resample_batch implements against
scipy.signal.resample_poly, the command line, the binding and the exported symbol."""
import ctypes

import numpy as np
import pytest
from scipy.signal import resample_poly

from f2cnn_amd import _lib, build, cli, resample


def formula(x, up, down, half_len, taps):
    """include/f2cnn_hip.h, f2_resample_batch step 2, term by term: product and sum rounded separately, ascending i"""
    n = len(x)
    n_out = -(-n * up // down)
    y = np.zeros(n_out)
    for k in range(n_out):
        c = k * down + half_len
        acc = 0.0
        for i in range(max(0, -(-(c - 2 * half_len) // up)), min(n - 1, c // up) + 1):
            acc = acc + x[i] * taps[c - i * up]
        y[k] = acc
    return y


@pytest.mark.parametrize("rate_in,rate_out", [(48000, 16000), (44100, 16000), (22050, 16000), (11025, 16000), (8000, 16000),
                                              (16000, 44100)])
def test_design_and_formula_reproduce_resample_poly(rate_in, rate_out):
    up, down, half_len, taps = resample.design_resampler(rate_in, rate_out)
    assert up * rate_in == down * rate_out and np.gcd(up, down) == 1
    assert half_len == 10 * max(up, down) and taps.shape == (2 * half_len + 1,) and taps.dtype == np.float64
    rng = np.random.default_rng(rate_in + rate_out)
    for n in (1, 3, 97, 1000):
        x = rng.integers(-32768, 32768, n).astype(np.float64)
        ref = resample_poly(x, rate_out, rate_in)
        got = formula(x, up, down, half_len, taps)
        assert got.shape == ref.shape == (_lib.resampled_length(n, up, down),)
        assert np.abs(got - ref).max() == 0.0, (rate_in, rate_out, n)


def test_equal_rates_are_the_conversion_alone():
    assert resample.design_resampler(16000, 16000)[:3] == (1, 1, 0)
    assert resample.design_resampler(44100, 44100)[:2] == (1, 1)


CNN_COMMANDS = ("eval", "evalnoise", "evalrand", "noisesweep")


def test_parser_accepts_resample_and_parses_as_before_without_it():
    parser = cli.build_parser()
    for command in CNN_COMMANDS:
        base = ["cnn", command, "--file", "a.WAV", "--hop", "frame"]
        without = parser.parse_args(base)
        assert "resample" not in vars(without)
        with_flag = parser.parse_args(base + ["--resample"])
        assert with_flag.resample is True
        rest = dict(vars(with_flag))
        del rest["resample"]
        assert rest == vars(without)
    # the namespace of a command line that worked before holds what it held
    assert vars(parser.parse_args(["cnn", "eval", "--file", "a.WAV"])) == dict(
        configure=False, file="a.WAV", inputFile=None, labelFile=None, model=None, cnn_command="eval", CUTOFF=None, count=None,
        SNRdB=None, hop=None, snrs=None, seed=None, save_wavs=False)


def test_binding_and_exported_symbol():
    res, args = _lib.SIGNATURES["f2_resample_batch"]
    assert res is ctypes.c_int and len(args) == 14
    lib = ctypes.CDLL(build.build_library())
    assert hasattr(lib, "f2_resample_batch")
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() >= 113


def test_dtype_to_pcm_format():
    want = {np.uint8: _lib.PCM_U8, np.int16: _lib.PCM_I16, np.int32: _lib.PCM_I32, np.float32: _lib.PCM_F32,
            np.float64: _lib.PCM_F64}
    assert (_lib.PCM_U8, _lib.PCM_I16, _lib.PCM_I32, _lib.PCM_F32, _lib.PCM_F64) == (0, 1, 2, 3, 4)
    for dtype, fmt in want.items():
        assert resample.pcm_format(dtype) == fmt and resample.pcm_format(np.dtype(dtype)) == fmt
    for dtype in (np.int8, np.int64, np.uint16, np.float16, np.complex128, bool):
        with pytest.raises(ValueError):
            resample.pcm_format(dtype)
    with pytest.raises(ValueError):
        resample.resample_arrays([np.zeros(4, np.int64)], 48000, 16000)
