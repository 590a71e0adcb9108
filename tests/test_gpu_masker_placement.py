"""The masker entries under the device-pointer contract of tests/test_gpu_device_placement.py: every device buffer at an odd
element misalignment between poisoned guard bands (tests/devmem.Arena), check() afterwards, the results bit for bit those of the
aligned call and of the host call. f2_masker_levels, f2_masker_pick, f2_eval_masker_sweep, f2_input_batch_masked; a render has no
device pointer of the caller's."""
import numpy as np
import pytest

import f2cnn_oracle as orc
import masker_cases as mc
import noisy_batch as nb
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel
from masker_cases import K, SEED
from test_gpu_device_placement import placed, same_bits
from test_gpu_shaped_noise import n_windows

pytestmark = pytest.mark.gpu

DEV, HOST = _lib.MEM_DEVICE, _lib.MEM_HOST
DTYPE = {_lib.WAVE_I16: np.int16, _lib.WAVE_F64: np.float64}
MASKERS, MASKER_OF, SNRS = mc.SETS["wraps"]
MISALIGNMENTS = ({"wave": 1, "noisy": 1}, {"wave": 3, "noisy": 5})


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_masker_levels(ctx, dt):
    flat, offsets = mc.ragged_waves()
    flat = flat.astype(DTYPE[dt])
    bufs = {"wave": (DTYPE[dt], len(flat), "in", flat), "noisy": (np.float64, (K + 1) * len(flat), "out", None)}

    def call(p):
        return ctx.masker_levels(p["wave"], dt, offsets, mc.B, SNRS, MASKERS, MASKER_OF, SEED, p["noisy"], DEV)
    ref, small = placed(ctx, bufs, {}, call)
    host = np.empty((K + 1) * len(flat))
    host_small = ctx.masker_levels(flat, dt, offsets, mc.B, SNRS, MASKERS, MASKER_OF, SEED, host, HOST)
    assert same_bits(ref["noisy"], host) and all(same_bits(a, b) for a, b in zip(small, host_small))
    for mis in MISALIGNMENTS:
        got, small1 = placed(ctx, bufs, mis, call)
        assert same_bits(got["noisy"], ref["noisy"]) and all(same_bits(a, b) for a, b in zip(small1, small)), mis


@pytest.mark.parametrize("dt", (_lib.WAVE_I16, _lib.WAVE_F64))
def test_masker_pick(ctx, dt):
    flat, offsets = mc.ragged_waves()
    flat = flat.astype(DTYPE[dt])
    level_of = (2, 5, 0, 4, 1, 3, 4)
    bufs = {"wave": (DTYPE[dt], len(flat), "in", flat), "noisy": (np.float64, len(flat), "out", None)}

    def call(p):
        return ctx.masker_pick(p["wave"], dt, offsets, mc.B, SNRS, MASKERS, MASKER_OF, level_of, 3, SEED, p["noisy"], DEV, small=True)
    ref, small = placed(ctx, bufs, {}, call)
    host = np.empty(len(flat))
    host_small = ctx.masker_pick(flat, dt, offsets, mc.B, SNRS, MASKERS, MASKER_OF, level_of, 3, SEED, host, HOST, small=True)
    assert same_bits(ref["noisy"], host) and all(same_bits(a, b) for a, b in zip(small, host_small))
    for mis in MISALIGNMENTS:
        got, small1 = placed(ctx, bufs, mis, call)
        assert same_bits(got["noisy"], ref["noisy"]) and all(same_bits(a, b) for a, b in zip(small1, small)), mis


def test_eval_masker_sweep(ctx):
    flat, offsets = mc.ragged_waves()
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, mc.C, 100))
    handle = F2CNNModel(orc.glorot_weights(7)).handle(ctx)
    nw = n_windows(mc.LENGTHS, mc.STEP, K + 1)
    bufs = {"wave": (np.int16, len(flat), "in", flat), "noisy": (np.float64, (K + 1) * len(flat), "out", None),
            "scores": (np.float32, 2 * nw, "out", None), "labels": (np.uint8, nw, "out", None)}

    def sweep(wave, noisy, scores, labels, mem):
        return ctx.eval_masker_sweep(handle, wave, _lib.WAVE_I16, offsets, coefs, mc.B, mc.C, False, 0.0, _lib.FFT_F32, mc.RADIUS, mc.STEP,
                                     mc.STEP, SNRS, MASKERS, MASKER_OF, SEED, noisy, scores, labels, mem)

    def call(p):
        return sweep(p["wave"], p["noisy"], p["scores"], p["labels"], DEV)
    ref, small = placed(ctx, bufs, {}, call)
    host = (np.empty((K + 1) * len(flat)), np.empty((nw, 2), np.float32), np.empty(nw, np.uint8))
    host_small = sweep(flat, *host, HOST)
    assert nw > 0 and all(same_bits(ref[name].reshape(h.shape), h) for name, h in zip(("noisy", "scores", "labels"), host))
    assert all(same_bits(a, b) for a, b in zip(small, host_small))
    for mis in ({"wave": 1, "noisy": 1, "scores": 1, "labels": 1}, {"wave": 3, "noisy": 3, "scores": 3, "labels": 7}):
        got, small1 = placed(ctx, bufs, mis, call)
        assert all(same_bits(got[name], ref[name]) for name in ref) and all(same_bits(a, b) for a, b in zip(small1, small)), mis


def test_input_batch_masked(ctx):
    dt = _lib.WAVE_I16
    flat, offsets = nb.waves(dt)
    coefs = nb.coefs()
    cs, coff = nb.centers()
    centres, nwin = np.concatenate(cs), int(coff[-1])
    masker_level_of = (3, 5, 0, 4, 2, 1)
    bufs = {"wave": (DTYPE[dt], len(flat), "in", flat), "windows": (np.float32, nwin * nb.R * nb.C, "out", None)}

    def call(p):
        ctx.input_batch_masked(p["wave"], dt, offsets, coefs, nb.B, nb.C, True, 50.0, _lib.FFT_F32, coff, centres, nb.RADIUS, nb.STEP, True, (), None,
                               nb.SNR, None, nb.LEVEL_OF, 0, nb.SEED, None, None, MASKERS, MASKER_OF, SNRS, masker_level_of, p["windows"], DEV)
    with ctx.options(spectral_min_rows=0):
        ref = placed(ctx, bufs, {}, call)[0]["windows"]
        assert np.isfinite(ref).all() and ref.min() >= 0 and ref.max() <= 1
        for mis in ({"wave": 1, "windows": 1}, {"wave": 3, "windows": 3}):
            got = placed(ctx, bufs, mis, call)[0]["windows"]
            assert same_bits(got, ref), mis
