"""f2_eval_masker_sweep: the levels of f2_masker_levels evaluated as one (K+1) * B batch. The waveforms and the small outputs on raw
bits against f2_masker_levels, the evaluation on raw bits against f2_eval_batch_strided(F2_WAVE_F64) on the waveforms the call
returns, the tally against counts made from the returned labels, and the batch without a window. The glorot model of
tests/test_gpu_shaped_noise.py, through the C ABI via ctypes."""
import numpy as np
import pytest

import f2cnn_oracle as orc
import masker_cases as mc
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel
from masker_cases import B, C, K, LENGTHS, RADIUS, SEED, STEP, bits, filled, ptr
from test_gpu_shaped_noise import n_windows, numpy_stats, tiled_offsets

pytestmark = pytest.mark.gpu

U = (K + 1) * B
NAMES = ("noisy", "scores", "labels", "wo", "sigma", "gain", "start", "stats")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))


@pytest.fixture(scope="module")
def model():
    return F2CNNModel(orc.glorot_weights(7))


class Out:
    """every output of one call, pre-filled with 0x5A"""

    def __init__(self, offsets, hop, levels=K + 1):
        lengths, nb = np.diff(offsets), len(offsets) - 1
        nw = n_windows(lengths, hop, levels)
        self.noisy = filled(levels * int(offsets[-1]), np.float64)
        self.scores, self.labels = filled((nw, 2), np.float32), filled(nw, np.uint8)
        self.wo = filled(levels * nb + 1, np.int64)
        self.sigma, self.gain, self.start = filled(levels * nb, np.float64), filled(levels * nb, np.float64), filled(levels * nb, np.int64)
        self.stats = filled((levels * nb, 2), np.int64)

    def untouched(self):
        return all((bits(getattr(self, name)) == mc.FILL).all() for name in NAMES)


def raw_sweep(ctx, model, coefs, wave, offsets, hop, snr, masker, moff, r, mof, k, o):
    return ctx.lib.f2_eval_masker_sweep(ctx.handle, model.handle(ctx), ptr(wave), _lib.WAVE_I16, ptr(offsets), ptr(coefs), len(offsets) - 1, C,
                                        0, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, ptr(snr), ptr(masker), ptr(moff), r, ptr(mof), k, SEED,
                                        ptr(o.noisy), ptr(o.scores), ptr(o.labels), ptr(o.wo), ptr(o.sigma), ptr(o.gain), ptr(o.start),
                                        ptr(o.stats), _lib.MEM_HOST)


def sweep(ctx, model, coefs, wave, offsets, hop, name="wraps"):
    recordings, masker_of, snr = mc.SETS[name]
    masker, moff = _lib._pack_rirs(recordings)
    o = Out(offsets, hop)
    rc = raw_sweep(ctx, model, coefs, wave, offsets, hop, np.array(snr, np.float64), masker, moff, len(recordings), np.array(masker_of, np.int32),
                   K, o)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return o


@pytest.fixture(scope="module")
def frame_sweep(ctx, model, coefs):
    wave, offsets = mc.ragged_waves()
    return sweep(ctx, model, coefs, wave, offsets, STEP)


def test_waveforms_and_small_outputs_are_f2_masker_levels(ctx, frame_sweep):
    wave, offsets = mc.ragged_waves()
    recordings, masker_of, snr = mc.SETS["wraps"]
    noisy = filled((K + 1) * int(offsets[-1]), np.float64)
    sigma, gain, start = ctx.masker_levels(wave, _lib.WAVE_I16, offsets, B, snr, recordings, masker_of, SEED, noisy, _lib.MEM_HOST)
    for name, want in (("noisy", noisy), ("sigma", sigma), ("gain", gain), ("start", start)):
        assert bits(getattr(frame_sweep, name)).tobytes() == bits(want).tobytes(), name
    assert (gain.reshape(K + 1, B)[:K, 2:] > 0).all()


@pytest.mark.parametrize("hop", (1, STEP))
def test_evaluation_is_the_strided_call_on_the_returned_waveforms(ctx, model, coefs, frame_sweep, hop):
    wave, offsets = mc.ragged_waves()
    o = frame_sweep if hop == STEP else sweep(ctx, model, coefs, wave, offsets, hop)
    nw = n_windows(LENGTHS, hop, K + 1)
    sc, lb = filled((nw, 2), np.float32), filled(nw, np.uint8)
    wo = ctx.eval_batch_strided(model.handle(ctx), o.noisy, _lib.WAVE_F64, tiled_offsets(offsets, K + 1), coefs, U, C, False, 0.0, _lib.FFT_F32,
                                RADIUS, STEP, hop, sc, lb, _lib.MEM_HOST)
    assert np.array_equal(o.wo, wo) and o.wo[-1] == nw > 0
    assert bits(o.scores).tobytes() == bits(sc).tobytes()
    assert np.array_equal(o.labels, lb) and set(np.unique(o.labels)) <= {0, 1}
    assert np.array_equal(o.stats, numpy_stats(o.labels, o.wo, K, B))
    assert np.array_equal(o.stats[K * B:, 1], np.diff(o.wo)[K * B:])                   # the clean level agrees with itself
    if hop == 1:
        assert bits(o.noisy).tobytes() == bits(frame_sweep.noisy).tobytes()            # the waveforms do not depend on the hop


def test_a_batch_without_a_window_fills_the_small_outputs(ctx, model, coefs):
    lengths = (0, 1, 1025, 1760)
    wave, offsets = mc.ragged_waves(lengths)
    o = sweep(ctx, model, coefs, wave, offsets, STEP, "silent")
    nb = len(lengths)
    assert (o.wo == 0).all() and (o.stats == 0).all() and len(o.scores) == 0
    recordings, masker_of, snr = mc.SETS["silent"]
    noisy = filled((K + 1) * int(offsets[-1]), np.float64)
    sigma, gain, start = ctx.masker_levels(wave, _lib.WAVE_I16, offsets, nb, snr, recordings, masker_of, SEED, noisy, _lib.MEM_HOST)
    for name, want in (("noisy", noisy), ("sigma", sigma), ("gain", gain), ("start", start)):
        assert bits(getattr(o, name)).tobytes() == bits(want).tobytes(), name
    # ... and a batch without a sample: zeros, and the waveform buffer is not needed
    empty = Out(np.zeros(3, np.int64), STEP)
    masker, moff = _lib._pack_rirs(recordings)
    rc = raw_sweep(ctx, model, coefs, None, np.zeros(3, np.int64), STEP, np.array(snr, np.float64), masker, moff, len(recordings),
                   np.array(masker_of, np.int32), K, empty)
    assert rc == _lib.F2_OK
    assert all((getattr(empty, name) == 0).all() for name in ("wo", "sigma", "gain", "start", "stats"))


def test_errors_of_the_maskers_come_before_anything_is_written(ctx, model, coefs):
    wave, offsets = mc.ragged_waves()
    recordings, masker_of, snr = mc.SETS["wraps"]
    masker, moff = _lib._pack_rirs(recordings)
    o = Out(offsets, STEP)
    nan = masker.copy()
    nan[5] = np.nan
    bad_of = np.array(masker_of, np.int32)
    bad_of[1] = 9
    good = dict(snr=np.array(snr, np.float64), masker=masker, moff=moff, r=len(recordings), mof=np.array(masker_of, np.int32), k=K)
    for kw, status, word in ((dict(masker=nan), _lib.F2_ERR_INVALID, "recording 1: sample 4"), (dict(mof=bad_of), _lib.F2_ERR_INVALID, "level 1"),
                             (dict(masker=None), _lib.F2_ERR_INVALID, "masker"), (dict(r=65), _lib.F2_ERR_UNSUPPORTED, "65 recordings"),
                             (dict(k=0), _lib.F2_ERR_INVALID, "K=0")):
        assert raw_sweep(ctx, model, coefs, wave, offsets, STEP, o=o, **{**good, **kw}) == status, list(kw)
        assert word in ctx.lib.f2_last_error(ctx.handle).decode(), list(kw)
        assert o.untouched(), list(kw)
