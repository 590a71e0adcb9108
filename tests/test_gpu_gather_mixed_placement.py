"""f2_gather_windows_mixed and f2_input_batch_smeared under the device-pointer contract of tests/test_gpu_device_placement.py: every
device buffer at an odd element misalignment between poisoned guard bands (tests/devmem.Arena), check() afterwards, the results
bit for bit those of the aligned call and of the host call. The kernel reads env one float64 and writes windows one float32 per
access: element alignment is all it needs."""
import numpy as np
import pytest

import noisy_batch as nb
import test_gpu_gather_mixed as gm
from f2cnn_amd import _lib
from test_gpu_device_placement import placed, same_bits

pytestmark = pytest.mark.gpu

DEV = _lib.MEM_DEVICE


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("C,normalize", ((33, 1), (128, 1), (128, 0)))
def test_gather_windows_mixed(ctx, C, normalize):
    radius, step = 5, 16
    env, mix = gm.envelopes(C), gm.matrices(C)
    cs, coff = gm.centres(radius, step)
    cen, nwin, R = np.concatenate(cs), int(coff[-1]), 2 * radius + 1
    bufs = {"env": (np.float64, len(env), "in", env), "windows": (np.float32, nwin * R * C, "out", None)}

    def call(p):
        ctx.gather_windows_mixed(p["env"], gm.OFFSETS, gm.B, C, coff, cen, radius, step, normalize, mix, gm.MIX_OF, p["windows"], DEV)
    ref = placed(ctx, bufs, {}, call)[0]["windows"]
    host = gm.mixed(ctx, env, C, gm.OFFSETS, cs, coff, radius, step, normalize, mix, gm.MIX_OF)
    assert same_bits(ref.reshape(host.shape), host)
    for mis in ({"env": 1, "windows": 1}, {"env": 5, "windows": 3}, {"env": 15, "windows": 31}):
        got = placed(ctx, bufs, mis, call)[0]["windows"]
        assert same_bits(got, ref), mis


def test_input_batch_smeared(ctx):
    dt = _lib.WAVE_I16
    flat, offsets = nb.waves(dt)
    coefs = nb.coefs()
    cs, coff = nb.centers()
    centres, nwin = np.concatenate(cs), int(coff[-1])
    mix = gm.matrices(nb.C)
    mix_of = (0, 4, 1, 3, 2, 4)
    bufs = {"wave": (np.int16, len(flat), "in", flat), "windows": (np.float32, nwin * nb.R * nb.C, "out", None)}

    def call(p):
        ctx.input_batch_smeared(p["wave"], dt, offsets, coefs, nb.B, nb.C, True, 50.0, _lib.FFT_F32, coff, centres, nb.RADIUS, nb.STEP, True,
                                (), None, nb.SNR, None, nb.LEVEL_OF, 0, nb.SEED, mix, mix_of, p["windows"], DEV)
    with ctx.options(spectral_min_rows=0):
        ref = placed(ctx, bufs, {}, call)[0]["windows"]
        assert np.isfinite(ref).all() and ref.min() >= 0 and ref.max() <= 1
        for mis in ({"wave": 1, "windows": 1}, {"wave": 3, "windows": 3}):
            got = placed(ctx, bufs, mis, call)[0]["windows"]
            assert same_bits(got, ref), mis
