"""f2_cnn_input_gradient, f2_saliency_map and f2_eval_saliency_batch with F2_MEM_DEVICE buffers at placements a caller's tensor
slice produces, as tests/test_gpu_smear_sweep_placement.py holds the sweeps: every buffer inside one arena (tests/devmem.py)
between guard bands of poison, a number of elements past a 256-byte boundary. Asserted per placement: the outputs equal the
host-memory call on raw bits, every guard band and every input is byte for byte as before, no output element keeps its pre-fill.

What the new kernels do to caller-supplied pointers: k_conv1_fwd and k_grad_profile load x, and k_conv1_bwd stores G, one float32
per lane; the scores arrive by a device-to-device copy; k_grad_profile and k_saliency_map load and store single float64 values -
element alignment, as the header grants. The 16-byte accesses of the chain are all inside its own scratch."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from devmem import Arena
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

I16, F64, F32, U8 = np.int16, np.float64, np.float32, np.uint8
RADIUS, STEP, R = 5, 160, 11
DEV, HOST = _lib.MEM_DEVICE, _lib.MEM_HOST
C = 16


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model():
    return F2CNNModel.glorot(7, R, C, zero_bias=False)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def placed(ctx, bufs, mis, call):
    """One call at one placement. bufs: {name: (dtype, count, role, data or None)}; mis: {name: misalign}, 0 where not named.
    Returns ({name: array} of the out regions, what `call` returned)."""
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
        for name, (dt, _, role, _) in bufs.items():
            if role == "out":
                if dt != U8:      # (a picture level may be the poison byte by right: those are held by the comparison with the host call)
                    assert a.unwritten(name) == 0, f"{a.unwritten(name)} elements of '{name}' were never written"
                outs[name] = a.download(name)
        return outs, extra


# ---- f2_cnn_input_gradient ----------------------------------------------------------------------------------------------------------------
N = 67


@pytest.fixture(scope="module")
def gradient_case(ctx, model):
    x = np.random.default_rng(3).random((N, R, C)).astype(F32)
    G, profile, scores = np.empty((N, R, C), F32), np.empty((N, C, 2)), np.empty((N, 2), F32)
    ctx.cnn_input_gradient(model.handle(ctx), x, N, G, profile, scores, HOST)
    assert np.abs(G).max() > 0
    for a in (x, G, profile, scores):
        a.setflags(write=False)
    return dict(x=x, grad=G, profile=profile, scores=scores)


@pytest.mark.parametrize("mis", [dict(), dict(x=1, grad=1, profile=1, scores=1), dict(x=3, grad=0, profile=15, scores=1),
                                 dict(x=0, grad=3, profile=0, scores=0)], ids=["aligned", "1", "3-0-15-1", "0-3-0-0"])
def test_input_gradient(ctx, model, gradient_case, mis):
    s = gradient_case
    bufs = {"x": (F32, s["x"].size, "in", s["x"]), "grad": (F32, s["grad"].size, "out", None),
            "profile": (F64, s["profile"].size, "out", None), "scores": (F32, s["scores"].size, "out", None)}
    got, _ = placed(ctx, bufs, mis, lambda p: ctx.cnn_input_gradient(model.handle(ctx), p["x"], N, p["grad"], p["profile"], p["scores"], DEV))
    for k in ("grad", "profile", "scores"):
        assert same_bits(got[k], s[k]), k


def test_input_gradient_with_outputs_left_out(ctx, model, gradient_case):
    """device memory, NULL gradient: G lives in the chain's scratch, the profile is still formed from it"""
    s = gradient_case
    bufs = {"x": (F32, s["x"].size, "in", s["x"]), "profile": (F64, s["profile"].size, "out", None)}
    got, _ = placed(ctx, bufs, dict(x=1, profile=1), lambda p: ctx.cnn_input_gradient(model.handle(ctx), p["x"], N, None, p["profile"], None, DEV))
    assert same_bits(got["profile"], s["profile"])


# ---- f2_saliency_map ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_mis,m_mis", [(0, 0), (1, 1), (15, 1), (1, 7)])
def test_saliency_map(ctx, p_mis, m_mis):
    rows = (0, 1, 37, 2000)
    wo = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    hop, W, origin = 7, 50, 800
    spans = np.array([[0, 2 * origin + n * hop] for n in rows], np.int64)
    profile = np.random.default_rng(8).standard_normal((int(wo[-1]), C, 2))
    host = ctx.saliency_map(profile, wo, C, spans, origin, hop, W, np.empty((len(rows), C, W, 3)), HOST)
    bufs = {"profile": (F64, profile.size, "in", profile), "map": (F64, host.size, "out", None)}
    got, _ = placed(ctx, bufs, dict(profile=p_mis, map=m_mis),
                    lambda p: ctx.saliency_map(p["profile"], wo, C, spans, origin, hop, W, p["map"], DEV))
    assert same_bits(got["map"], host)


# ---- f2_eval_saliency_batch ---------------------------------------------------------------------------------------------------------------
LENS = [2500, 1761, 3001, 1700]
W = 40


@pytest.fixture(scope="module")
def eval_case(ctx, model):
    freqs = filters.centre_freqs(16000, C, 100)
    coefs = np.ascontiguousarray(filters.make_erb_filters(16000, freqs))
    waves = [orc.synth_utterance(3100 + i, n) for i, n in enumerate(LENS)]
    off, flat = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64), np.concatenate(waves).astype(I16)
    hop, B = 16, len(LENS)
    nwin = sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in LENS)
    o = dict(levels=np.empty((B, C, W), U8), map=np.empty((B, C, W, 3)), summary=np.empty((B, C, 3)), scores=np.empty((nwin, 2), F32),
             labels=np.empty(nwin, U8))
    wo, rng = ctx.eval_saliency_batch(model.handle(ctx), flat, _lib.WAVE_I16, off, coefs, B, C, True, 50.0, _lib.FFT_F32, RADIUS, STEP, hop,
                                      None, W, 0, o["levels"], o["map"], o["summary"], o["scores"], o["labels"], HOST)
    assert wo[-1] == nwin > 0 and wo[-1] == wo[-2]
    for a in list(o.values()) + [flat, wo]:
        a.setflags(write=False)
    return dict(o, coefs=coefs, off=off, flat=flat, hop=hop, nwin=nwin, wo=wo, range=rng.copy())


@pytest.mark.parametrize("mis", [dict(), dict(wave=1, levels=1, map=1, summary=1, scores=1, labels=1),
                                 dict(wave=1, levels=3, map=15, summary=0, scores=0, labels=1)], ids=["aligned", "1", "mixed"])
def test_eval_saliency_batch(ctx, model, eval_case, mis):
    s = eval_case
    B = len(LENS)
    bufs = {"wave": (I16, len(s["flat"]), "in", s["flat"]), "levels": (U8, s["levels"].size, "out", None),
            "map": (F64, s["map"].size, "out", None), "summary": (F64, s["summary"].size, "out", None),
            "scores": (F32, 2 * s["nwin"], "out", None), "labels": (U8, s["nwin"], "out", None)}

    def call(p):
        return ctx.eval_saliency_batch(model.handle(ctx), p["wave"], _lib.WAVE_I16, s["off"], s["coefs"], B, C, True, 50.0, _lib.FFT_F32,
                                       RADIUS, STEP, s["hop"], None, W, 0, p["levels"], p["map"], p["summary"], p["scores"], p["labels"], DEV)
    got, (wo, rng) = placed(ctx, bufs, mis, call)
    assert np.array_equal(wo, s["wo"]) and same_bits(rng, s["range"])
    for k in ("levels", "map", "summary", "scores", "labels"):
        assert same_bits(got[k], s[k]), k
