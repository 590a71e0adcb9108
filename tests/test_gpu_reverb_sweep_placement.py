"""f2_reverb_levels and f2_eval_reverb_sweep with F2_MEM_DEVICE buffers at placements a caller's tensor slice produces, as
tests/test_gpu_cutoff_sweep_placement.py holds the cutoff sweep: every buffer inside one arena (tests/devmem.py) between guard
bands of poison, 0, 1 or 3 elements past a 256-byte boundary. Asserted per placement: the outputs equal the host-memory call on
raw bits, every guard band and every input is byte for byte as before, no output element keeps its pre-fill.

What the new kernel does to caller-supplied pointers: k_reverb_levels loads single int16 / float64 samples and stores single
float64 values, four in a row per lane, guarded one by one at an utterance's end - element alignment, as the header grants."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from devmem import Arena
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.reverb import SyntheticRIR

pytestmark = pytest.mark.gpu

I16, F64, F32, U8 = np.int16, np.float64, np.float32, np.uint8
RADIUS, STEP = 5, 160
DEV, HOST = _lib.MEM_DEVICE, _lib.MEM_HOST
C = 40
BLK, TC = _lib.REVERB_BLOCK, _lib.REVERB_TAP_CHUNK
RIRS = (np.array([1.0]), SyntheticRIR(1.0, 257, seed=2, level=1), SyntheticRIR(1.0, TC + 5, seed=2, level=2))
K = len(RIRS)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def placed(ctx, bufs, mis, call):
    """One call at one placement, as tests/test_gpu_device_placement.py places it. bufs: {name: (dtype, count, role, data or
    None)}; mis: {name: misalign}, 0 where not named. Returns ({name: array} of the out regions, what `call` returned)."""
    with Arena(ctx) as a:
        for name, (dt, count, role, _) in bufs.items():
            a.region(name, dt, count, misalign=mis.get(name, 0), role=role)
        for name, (_, _, _, data) in bufs.items():
            if data is not None:
                a.upload(name, data)
        extra = call({name: a.ptr(name) for name in bufs})
        ctx.synchronize()
        a.check()
        outs = {}
        for name, (_, _, role, _) in bufs.items():
            if role == "out":
                assert a.unwritten(name) == 0, f"{a.unwritten(name)} elements of '{name}' were never written"
                outs[name] = a.download(name)
        return outs, extra


# ---- f2_reverb_levels -------------------------------------------------------------------------------------------------------
RV_LENS = [65, 1, BLK + 1, 0, 2, BLK - 1, 63]          # odd lengths: utterances start at odd elements; the output tile's edge


@pytest.fixture(scope="module")
def levels_case(ctx):
    off = offsets_of(RV_LENS)
    rng = np.random.default_rng(9)
    wave = {I16: rng.integers(-32768, 32768, int(off[-1])).astype(I16), F64: rng.standard_normal(int(off[-1])) * 1000.0}
    host = {}
    for dt, w in wave.items():
        host[dt] = np.empty((K + 1) * w.size)
        ctx.reverb_levels(w, _lib.WAVE_I16 if dt is I16 else _lib.WAVE_F64, off, len(RV_LENS), RIRS, host[dt], HOST)
        w.setflags(write=False)
        host[dt].setflags(write=False)
    return off, wave, host


@pytest.mark.parametrize("dt", [I16, F64], ids=["int16", "float64"])
@pytest.mark.parametrize("wave_mis,lev_mis", [(0, 0), (1, 1), (3, 3), (1, 3), (3, 0)])
def test_reverb_levels(ctx, levels_case, dt, wave_mis, lev_mis):
    off, wave, host = levels_case
    w, want = wave[dt], host[dt]
    code = _lib.WAVE_I16 if dt is I16 else _lib.WAVE_F64
    bufs = {"wave": (dt, w.size, "in", w), "levels": (F64, want.size, "out", None)}
    got, _ = placed(ctx, bufs, dict(wave=wave_mis, levels=lev_mis),
                    lambda p: ctx.reverb_levels(p["wave"], code, off, len(RV_LENS), RIRS, p["levels"], DEV))
    assert same_bits(got["levels"], want)
    assert same_bits(got["levels"][K * w.size:], w.astype(F64))


# ---- f2_eval_reverb_sweep ---------------------------------------------------------------------------------------------------
SW_LENS = [2500, 1761, 3001]


@pytest.fixture(scope="module")
def sweep_case(ctx):
    """the batch, its network and the host-memory call: computed once, only read"""
    model = F2CNNModel.glorot(7, 11, C)
    coefs = filters.make_erb_filters(16000, filters.centre_freqs(16000, C, 100))
    waves = [orc.synth_utterance(3100 + i, n) for i, n in enumerate(SW_LENS)]
    off, flat = offsets_of(SW_LENS), np.concatenate(waves)
    hop = 16
    nwin = (K + 1) * sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in SW_LENS)
    wet, scores, labels = np.empty((K + 1) * len(flat)), np.empty((nwin, 2), F32), np.empty(nwin, U8)
    wo, stats = ctx.eval_reverb_sweep(model.handle(ctx), flat, _lib.WAVE_I16, off, coefs, len(SW_LENS), C, False, 0.0, _lib.FFT_F32,
                                      RADIUS, STEP, hop, RIRS, wet, scores, labels, HOST)
    assert wo[-1] == nwin > 0
    for a in (wet, scores, labels, wo, stats, flat):
        a.setflags(write=False)
    return dict(model=model, coefs=coefs, off=off, flat=flat, hop=hop, nwin=nwin, wet=wet, scores=scores, labels=labels, wo=wo,
                stats=stats)


@pytest.mark.parametrize("mis", [dict(), dict(wave=1, wet=1, scores=1, labels=1), dict(wave=3, wet=3, scores=3, labels=3),
                                 dict(wave=1, wet=3, scores=1, labels=3)], ids=["aligned", "1", "3", "1-3-1-3"])
def test_reverb_sweep(ctx, sweep_case, mis):
    s = sweep_case
    h = s["model"].handle(ctx)
    bufs = {"wave": (I16, len(s["flat"]), "in", s["flat"]), "wet": (F64, s["wet"].size, "out", None),
            "scores": (F32, 2 * s["nwin"], "out", None), "labels": (U8, s["nwin"], "out", None)}

    def call(p):
        return ctx.eval_reverb_sweep(h, p["wave"], _lib.WAVE_I16, s["off"], s["coefs"], len(SW_LENS), C, False, 0.0, _lib.FFT_F32, RADIUS,
                                     STEP, s["hop"], RIRS, p["wet"], p["scores"], p["labels"], DEV)
    got, (wo, stats) = placed(ctx, bufs, mis, call)
    assert np.array_equal(wo, s["wo"]) and np.array_equal(stats, s["stats"])
    for k in ("wet", "scores", "labels"):
        assert same_bits(got[k], s[k]), k


def test_reverb_sweep_with_outputs_left_out(ctx, sweep_case):
    """device memory, NULL: the wet waveforms and the labels live in context scratch, the tally still counts them"""
    s = sweep_case
    h = s["model"].handle(ctx)
    bufs = {"wave": (I16, len(s["flat"]), "in", s["flat"]), "scores": (F32, 2 * s["nwin"], "out", None)}

    def call(p):
        return ctx.eval_reverb_sweep(h, p["wave"], _lib.WAVE_I16, s["off"], s["coefs"], len(SW_LENS), C, False, 0.0, _lib.FFT_F32, RADIUS,
                                     STEP, s["hop"], RIRS, None, p["scores"], None, DEV)
    got, (wo, stats) = placed(ctx, bufs, dict(wave=1, scores=1), call)
    assert np.array_equal(wo, s["wo"]) and np.array_equal(stats, s["stats"]) and same_bits(got["scores"], s["scores"])
