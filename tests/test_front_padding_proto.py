"""The formulation the spectral kernels use for rows of up to 32768 samples - row padded IN FRONT, no end-of-row phase factor on
the ringing term (tests/diag/proto_front_padding.py, float32 emulation on the CPU) - against the oracle and against the
back-padded formulation (tests/diag/proto_spectral.py). Bounds: both formulations sit at 1.4e-7 .. 4.7e-7 of the row maximum
against the oracle on noise and on a low sine, and differ from each other by at most 5.2e-7: 1e-6."""
import os
import sys

import numpy as np
import pytest

import f2cnn_oracle as orc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "diag"))
import proto_front_padding as pf   # noqa: E402

BOUND = 1e-6


@pytest.mark.parametrize("n", [4097, 5000, 7937])
def test_front_padding_matches_the_oracle_and_the_back_padded_form(n):
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, 128, 100))[[0, 40, 127]]
    x = orc.synth_utterance(4000 + n, n).astype(np.float64)
    front, back, front_back, pad = pf.compare(x, coefs)
    print(f"n {n}: front {front:.2e}, back {back:.2e}, front against back {front_back:.2e}, padding residual {pad:.2e}")
    assert front <= BOUND
    assert front_back <= BOUND
