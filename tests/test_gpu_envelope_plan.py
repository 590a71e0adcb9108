"""K2's choice of radix plan for rows of 8193..16384 samples (H = 8192): three passes without the float low-pass unless the
context option env_plan4 forces four, four passes with it - both plans against the oracle, and bit-identical results where
the option cannot change the kernel."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from conftest import chan_relerr
from f2cnn_amd import _lib
from f2cnn_amd.scripts.processing import EnvelopeExtraction as EE
from test_gpu_envelope import TOL, TOL_F64

pytestmark = pytest.mark.gpu

IN_CLASS = (8193, 16384)      # the two ends of the H = 8192 class: the most padding, none
OUTSIDE = 5000                # H = 4096: no plan to choose


@pytest.fixture(scope="module")
def rows():
    """{N: (matrix, {lpf: oracle envelope})}"""
    out = {}
    for N in IN_CLASS + (OUTSIDE,):
        m = np.random.default_rng(N).standard_normal((3, N)) * np.array([[1.0], [1e-6], [3000.0]])
        out[N] = (m, {lpf: orc.extract_envelope_from_matrix(m, lpf, 50) for lpf in (False, True)})
    return out


@pytest.mark.parametrize("precision,tol", [(_lib.FFT_F32, TOL), (_lib.FFT_F64, TOL_F64)])
@pytest.mark.parametrize("lpf", [False, True])
@pytest.mark.parametrize("N", IN_CLASS + (OUTSIDE,))
def test_both_plans(rows, N, lpf, precision, tol):
    m, ref = rows[N]
    ctx = _lib.default_context()
    got = {}
    for plan4 in (0, 1):
        with ctx.options(env_plan4=plan4):
            got[plan4] = EE.ExtractEnvelopeFromMatrix(m, lpf, 50, precision=precision)
        assert chan_relerr(got[plan4], ref[lpf]) <= tol, (N, lpf, plan4)
    if N == OUTSIDE or (lpf and precision == _lib.FFT_F32):
        # the rule picks the same kernel for either value of the option
        assert np.array_equal(got[0], got[1])
