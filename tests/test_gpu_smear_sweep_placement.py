"""f2_channel_mix_levels and f2_eval_smear_sweep with F2_MEM_DEVICE buffers at placements a caller's tensor slice produces, as
tests/test_gpu_cutoff_sweep_placement.py holds the cutoff sweep: every buffer inside one arena (tests/devmem.py) between guard
bands of poison, a number of elements past a 256-byte boundary. Asserted per placement: the outputs equal the host-memory call on
raw bits, every guard band and every input is byte for byte as before, no output element keeps its pre-fill.

What the new kernel does to caller-supplied pointers: k_channel_mix_levels loads and stores single float64 values, consecutive
lanes at consecutive doubles - element alignment, as the header grants; a lane past the end of a short utterance re-reads the
utterance's last sample and stores nothing. Misalignments 0 and 1 for every buffer, and 15 doubles (120 bytes: a wave's 512-byte
access there straddles the 128-byte lines) for the two float64 ones."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from devmem import Arena
from f2cnn_amd import _lib, smear
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

I16, F64, F32, U8 = np.int16, np.float64, np.float32, np.uint8
RADIUS, STEP = 5, 160
DEV, HOST = _lib.MEM_DEVICE, _lib.MEM_HOST
TS, TC = _lib.SMEAR_TILE_SAMPLES, _lib.SMEAR_TILE_CHANNELS


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


# ---- f2_channel_mix_levels ----------------------------------------------------------------------------------------------------------------
CM_C = TC + 1                                                  # two channel tiles, the second with one row
CM_LENS = [65, 1, TS + 1, 0, 2, 2 * TS + 1, TS - 1, TS]        # odd lengths: rows start at odd 8-byte offsets; the tile edge


def cm_matrices():
    rng = np.random.default_rng(4)
    c = np.arange(CM_C)
    dense = rng.standard_normal((CM_C, CM_C))
    band = dense * (np.abs(c[:, None] - c[None, :]) <= 1 + c[:, None] % 3)
    corner = np.zeros((CM_C, CM_C))
    corner[0, CM_C - 1], corner[CM_C - 1, 0] = 2.0, -3.0
    return np.stack([dense, band, corner, np.eye(CM_C)])


@pytest.mark.parametrize("env_mis,lev_mis", [(0, 0), (1, 1), (0, 1), (1, 0), (15, 1), (1, 15)])
def test_channel_mix_levels(ctx, env_mis, lev_mis):
    off = offsets_of(CM_LENS)
    mix = cm_matrices()
    K = len(mix)
    env = np.random.default_rng(9).standard_normal(CM_C * int(off[-1]))
    host = np.empty((K + 1) * env.size)
    ctx.channel_mix_levels(env, off, len(CM_LENS), CM_C, mix, host, HOST)
    bufs = {"env": (F64, env.size, "in", env), "levels": (F64, host.size, "out", None)}
    got, _ = placed(ctx, bufs, dict(env=env_mis, levels=lev_mis),
                    lambda p: ctx.channel_mix_levels(p["env"], off, len(CM_LENS), CM_C, mix, p["levels"], DEV))
    assert same_bits(got["levels"], host)
    assert same_bits(got["levels"][K * env.size:], env)
    assert same_bits(got["levels"][(K - 1) * env.size:K * env.size], env)      # the identity (no -0.0 in this input)


# ---- f2_eval_smear_sweep ------------------------------------------------------------------------------------------------------------------
C = 16
SW_LENS = [2500, 1761, 3001]


@pytest.fixture(scope="module")
def sweep_case(ctx):
    """the batch, its network and the host-memory call: computed once, only read"""
    model = F2CNNModel.glorot(7, 11, C)
    freqs = filters.centre_freqs(16000, C, 100)
    coefs = np.ascontiguousarray(filters.make_erb_filters(16000, freqs))
    mix = np.stack([smear.SmearMatrix(freqs, 2.0), smear.BandMatrix(C, 4), smear.BandMatrix(C, C)])
    K = len(mix)
    waves = [orc.synth_utterance(3100 + i, n) for i, n in enumerate(SW_LENS)]
    off, flat = offsets_of(SW_LENS), np.concatenate(waves).astype(I16)
    hop = 16
    nwin = (K + 1) * sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in SW_LENS)
    env, scores, labels = np.empty((K + 1) * C * len(flat)), np.empty((nwin, 2), F32), np.empty(nwin, U8)
    wo, stats = ctx.eval_smear_sweep(model.handle(ctx), flat, _lib.WAVE_I16, off, coefs, len(SW_LENS), C, True, 50.0, _lib.FFT_F32, RADIUS,
                                     STEP, hop, mix, env, scores, labels, HOST)
    assert wo[-1] == nwin > 0
    for a in (env, scores, labels, wo, stats, flat):
        a.setflags(write=False)
    return dict(model=model, coefs=coefs, off=off, flat=flat, hop=hop, nwin=nwin, mix=mix, env=env, scores=scores, labels=labels, wo=wo,
                stats=stats)


@pytest.mark.parametrize("mis", [dict(), dict(wave=1, env=1, scores=1, labels=1), dict(wave=1, env=0, scores=0, labels=1),
                                 dict(wave=0, env=15, scores=1, labels=0)], ids=["aligned", "1", "1-0-0-1", "0-15-1-0"])
def test_smear_sweep(ctx, sweep_case, mis):
    s = sweep_case
    h = s["model"].handle(ctx)
    bufs = {"wave": (I16, len(s["flat"]), "in", s["flat"]), "env": (F64, s["env"].size, "out", None),
            "scores": (F32, 2 * s["nwin"], "out", None), "labels": (U8, s["nwin"], "out", None)}

    def call(p):
        return ctx.eval_smear_sweep(h, p["wave"], _lib.WAVE_I16, s["off"], s["coefs"], len(SW_LENS), C, True, 50.0, _lib.FFT_F32, RADIUS,
                                    STEP, s["hop"], s["mix"], p["env"], p["scores"], p["labels"], DEV)
    got, (wo, stats) = placed(ctx, bufs, mis, call)
    assert np.array_equal(wo, s["wo"]) and np.array_equal(stats, s["stats"])
    for k in ("env", "scores", "labels"):
        assert same_bits(got[k], s[k]), k


def test_smear_sweep_with_outputs_left_out(ctx, sweep_case):
    """device memory, NULL: the levels and the labels live in context scratch, the tally still counts them"""
    s = sweep_case
    h = s["model"].handle(ctx)
    bufs = {"wave": (I16, len(s["flat"]), "in", s["flat"]), "scores": (F32, 2 * s["nwin"], "out", None)}

    def call(p):
        return ctx.eval_smear_sweep(h, p["wave"], _lib.WAVE_I16, s["off"], s["coefs"], len(SW_LENS), C, True, 50.0, _lib.FFT_F32, RADIUS,
                                    STEP, s["hop"], s["mix"], None, p["scores"], None, DEV)
    got, (wo, stats) = placed(ctx, bufs, dict(wave=1, scores=1), call)
    assert np.array_equal(wo, s["wo"]) and np.array_equal(stats, s["stats"]) and same_bits(got["scores"], s["scores"])
