"""f2_reverb_pick and f2_input_batch_wet under the device-pointer contract of tests/test_gpu_device_placement.py: every device
buffer at an odd element misalignment between poisoned guard bands (tests/devmem.Arena), check() afterwards, the results bit for
bit those of the host-memory call."""
import numpy as np
import pytest

import noisy_batch as nb
from f2cnn_amd import _lib
from f2cnn_amd.reverb import SyntheticRIR
from noisy_batch import B, C, LEVEL_OF, R, RADIUS, SEED, SNR, STEP
from test_gpu_device_placement import placed, same_bits

pytestmark = pytest.mark.gpu

DEV = _lib.MEM_DEVICE
DTYPE = {_lib.WAVE_I16: np.int16, _lib.WAVE_F64: np.float64}
RIRS = [SyntheticRIR(1.0, t, seed=4, level=l) for l, t in enumerate((1, 1025, 2500))]
ROOM_OF = (1, 3, 0, 2, 0, 1)          # tests/noisy_batch.py's six utterances: every room and the dry one


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_reverb_pick(ctx, dt):
    flat, offsets = nb.waves(dt)
    bufs = {"wave": (DTYPE[dt], len(flat), "in", flat), "wet": (np.float64, len(flat), "out", None)}

    def call(p):
        ctx.reverb_pick(p["wave"], dt, offsets, B, RIRS, ROOM_OF, p["wet"], DEV)
    host = np.empty(len(flat))
    ctx.reverb_pick(flat, dt, offsets, B, RIRS, ROOM_OF, host, _lib.MEM_HOST)
    assert np.isfinite(host).all()
    for mis in ({}, {"wave": 1, "wet": 1}, {"wave": 3, "wet": 5}):
        got = placed(ctx, bufs, mis, call)[0]["wet"]
        assert same_bits(got, host), mis


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_input_batch_wet(ctx, dt):
    flat, offsets = nb.waves(dt)
    coefs = nb.coefs()
    cs, coff = nb.centers()
    centres, nwin = np.concatenate(cs), int(coff[-1])
    bufs = {"wave": (DTYPE[dt], len(flat), "in", flat), "windows": (np.float32, nwin * R * C, "out", None)}

    def call(p):
        ctx.input_batch_wet(p["wave"], dt, offsets, coefs, B, C, True, 50.0, _lib.FFT_F32, coff, centres, RADIUS, STEP, True, RIRS,
                            ROOM_OF, SNR, LEVEL_OF, 0, SEED, p["windows"], DEV)
    with ctx.options(spectral_min_rows=0):
        host = np.empty(nwin * R * C, np.float32)
        ctx.input_batch_wet(flat, dt, offsets, coefs, B, C, True, 50.0, _lib.FFT_F32, coff, centres, RADIUS, STEP, True, RIRS, ROOM_OF,
                            SNR, LEVEL_OF, 0, SEED, host, _lib.MEM_HOST)
        assert np.isfinite(host).all() and host.min() >= 0 and host.max() <= 1
        for mis in ({}, {"wave": 1, "windows": 1}, {"wave": 3, "windows": 3}):
            got = placed(ctx, bufs, mis, call)[0]["windows"]
            assert same_bits(got, host), mis
