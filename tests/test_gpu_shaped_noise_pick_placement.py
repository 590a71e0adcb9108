"""f2_shaped_noise_pick and f2_input_batch_coloured under the device-pointer contract of tests/test_gpu_device_placement.py: every
device buffer at an odd element misalignment between poisoned guard bands (tests/devmem.Arena), check() afterwards, the results
bit for bit those of the aligned call and of the host call."""
import numpy as np
import pytest

import noisy_batch as nb
from f2cnn_amd import _lib
from noisy_batch import B, C, LEVEL_OF, R, RADIUS, SEED, SNR, STEP
from test_gpu_device_placement import placed, same_bits
from test_gpu_shaped_noise import random_filter

pytestmark = pytest.mark.gpu

DEV = _lib.MEM_DEVICE
DTYPE = {_lib.WAVE_I16: np.int16, _lib.WAVE_F64: np.float64}
FIRS = [random_filter(t, 4) for t in (3, 1025, 2048)]      # tests/noisy_batch.py has three levels


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_shaped_noise_pick(ctx, dt):
    flat, offsets = nb.waves(dt)
    bufs = {"wave": (DTYPE[dt], len(flat), "in", flat), "noisy": (np.float64, len(flat), "out", None)}

    def call(p):
        return ctx.shaped_noise_pick(p["wave"], dt, offsets, B, SNR, FIRS, LEVEL_OF, 3, SEED, p["noisy"], DEV, sigma=True)
    ref, sigma = placed(ctx, bufs, {}, call)
    host = np.empty(len(flat))
    host_sigma = ctx.shaped_noise_pick(flat, dt, offsets, B, SNR, FIRS, LEVEL_OF, 3, SEED, host, _lib.MEM_HOST, sigma=True)
    assert same_bits(ref["noisy"], host) and same_bits(sigma, host_sigma)
    for mis in ({"wave": 1, "noisy": 1}, {"wave": 3, "noisy": 5}):
        got, sigma1 = placed(ctx, bufs, mis, call)
        assert same_bits(got["noisy"], ref["noisy"]) and same_bits(sigma1, sigma), mis


def test_input_batch_coloured(ctx):
    dt = _lib.WAVE_I16
    flat, offsets = nb.waves(dt)
    coefs = nb.coefs()
    cs, coff = nb.centers()
    centres, nwin = np.concatenate(cs), int(coff[-1])
    bufs = {"wave": (DTYPE[dt], len(flat), "in", flat), "windows": (np.float32, nwin * R * C, "out", None)}

    def call(p):
        ctx.input_batch_coloured(p["wave"], dt, offsets, coefs, B, C, True, 50.0, _lib.FFT_F32, coff, centres, RADIUS, STEP, True, (), None,
                                 SNR, FIRS, LEVEL_OF, 0, SEED, p["windows"], DEV)
    with ctx.options(spectral_min_rows=0):
        ref = placed(ctx, bufs, {}, call)[0]["windows"]
        assert np.isfinite(ref).all() and ref.min() >= 0 and ref.max() <= 1
        for mis in ({"wave": 1, "windows": 1}, {"wave": 3, "windows": 3}):
            got = placed(ctx, bufs, mis, call)[0]["windows"]
            assert same_bits(got, ref), mis
