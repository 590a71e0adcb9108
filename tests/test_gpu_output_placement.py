"""Where the outputs of the entry points live: every optional output present or NULL, in host and in device memory, gives the same
bits; a host call of more than one chunk equals the device call; different calls back to back on one context equal the same calls
on fresh contexts; contexts that keep the spectral guard's values come and go. The file records behaviour the library had before
its entry points shared one placement rule and one per-call meta area, and passes unchanged with that library.

Shapes are the smallest at which these paths can go wrong: radius 5, step 160, a ragged batch of 1761, 2500 and 1000 samples (one
window, several, none), 8 channels where no network is involved. The network is 11 x 10 with seeded Glorot weights, and the calls
that run it use 10 channels: 10 is the narrowest window f2_cnn_create accepts (conv - pool - conv - pool leaves ((C - 2) // 2 - 2)
// 2 columns, none for C = 8: an 11 x 8 network is an F2_ERR_INVALID).

Device buffers are regions of a tests/devmem.py arena: guard bands and inputs are checked after every call as well.
"""
import numpy as np
import pytest

import f2cnn_oracle as orc
from devmem import Arena
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.resample import design_resampler

pytestmark = pytest.mark.gpu

I16, F64, F32, U8, I32, I64 = np.int16, np.float64, np.float32, np.uint8, np.int32, np.int64
HOST, DEV = _lib.MEM_HOST, _lib.MEM_DEVICE
RADIUS, STEP, R, HOP = 5, 160, 11, 160
C_PIC, C_NET = 8, 10
LENS = [1761, 2500, 1000]
B = len(LENS)
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(I64)
TOTAL = int(OFFS[-1])
SNR, SEED = np.array([20.0, 5.0]), 1234
K = len(SNR)
U = (K + 1) * B
N_STRIDED = sum(_lib.strided_window_count(n, RADIUS, STEP, HOP) for n in LENS)    # 1 + 5 + 0
N_SWEEP = (K + 1) * N_STRIDED
N_UTT = LENS[1] - R * STEP       # every-sample windows of the 2500-sample utterance
WIDTH = 7
N_SCORE, GROUPS = 37, 3
P = _lib._ptr

_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def coefs(C):
    return once(("coefs", C), lambda: filters.make_erb_filters(16000, filters.centre_freqs(16000, C, 100)))


def wave():
    return once("wave", lambda: np.concatenate([orc.synth_utterance(900 + i, n) for i, n in enumerate(LENS)]))


def model():
    """a fresh object per context: F2CNNModel keeps its handles by id(ctx)"""
    return F2CNNModel.glorot(7, R, C_NET, zero_bias=False)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(U8), b.view(U8))


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def net(ctx):
    return model().handle(ctx)


class Call:
    """One entry point with its optional outputs. inputs: {name: array} (in the call's memory space); outputs: {name: (dtype,
    count, in_mem_space)} - in_mem_space False for the arrays that are host memory whatever the call's; make(ctx, h, a, mem): the
    call from a = {name: array | device pointer | None}, returning its mandatory results as a tuple of arrays."""

    def __init__(self, inputs, outputs, make):
        self.inputs, self.outputs, self.make = inputs, outputs, make

    def run(self, ctx, h, mem, present, arena=None, wait=True):
        """({name: array of every present output}, mandatory results); with `arena` (device memory; its regions are named
        <output>, <input>) the downloads are the caller's business when wait is False"""
        host = {k: np.zeros(n, dt) for k, (dt, n, in_mem) in self.outputs.items() if k in present and not (in_mem and mem == DEV)}
        if mem == HOST:
            a = dict(self.inputs)
            a.update({k: host.get(k) for k in self.outputs})
            return host, self.make(ctx, h, a, mem)
        own = arena is None
        arena = arena or Arena(ctx)
        try:
            if own:
                self.regions(arena, present)
                self.upload(arena)
            a = {k: arena.ptr(k) for k in self.inputs}
            a.update({k: host[k] if k in host else arena.ptr(k) if k in present else None for k in self.outputs})
            extra = self.make(ctx, h, a, mem)
            if not wait:
                return host, extra
            ctx.synchronize()
            arena.check()
            host.update(self.download(arena, present))
            return host, extra
        finally:
            if own:
                arena.free()

    def regions(self, arena, present, prefix=""):
        for k, v in self.inputs.items():
            arena.region(prefix + k, v.dtype, v.size, role="in")
        for k, (dt, n, in_mem) in self.outputs.items():
            if in_mem and k in present:
                arena.region(prefix + k, dt, n, role="out")

    def upload(self, arena, prefix=""):
        for k, v in self.inputs.items():
            arena.upload(prefix + k, v)

    def download(self, arena, present, prefix=""):
        return {k: arena.download(prefix + k) for k, (_, _, in_mem) in self.outputs.items() if in_mem and k in present}


def sweep_call():
    def make(ctx, h, a, mem):
        ctx.check(ctx.lib.f2_eval_noise_sweep(ctx.handle, h, P(a["wave"]), _lib.WAVE_I16, P(OFFS), P(coefs(C_NET)), B, C_NET, 1, 50.0,
                                              _lib.FFT_F32, RADIUS, STEP, HOP, P(SNR), K, SEED, P(a["noisy"]), P(a["scores"]),
                                              P(a["labels"]), P(a["window_offsets"]), P(a["sigma"]), P(a["stats"]), mem))
        return ()
    return Call({"wave": wave()}, {"noisy": (F64, (K + 1) * TOTAL, True), "scores": (F32, 2 * N_SWEEP, True), "labels": (U8, N_SWEEP, True),
                                   "window_offsets": (I64, U + 1, False), "sigma": (F64, U, False), "stats": (I64, 2 * U, False)}, make)


def score_inputs():
    rng = np.random.default_rng(5)
    return {"windows": rng.random((N_SCORE, R, C_NET)).astype(F32) + F32(0.5), "signs": (np.arange(N_SCORE) % 2).astype(U8),
            "groups": (np.arange(N_SCORE) % GROUPS).astype(I32)}


def score_call(normalize=1):
    def make(ctx, h, a, mem):
        counts, loss = ctx.cnn_score_windows(h, a["windows"], N_SCORE, normalize, a["signs"], a["groups"], GROUPS, a["scores"], a["labels"], mem)
        return counts, loss
    return Call(once("score_inputs", score_inputs), {"scores": (F32, 2 * N_SCORE, True), "labels": (U8, N_SCORE, True)}, make)


PIC_OUT = {"pooled": (F64, B * C_PIC * WIDTH, True), "levels": (U8, B * C_PIC * WIDTH, True), "range": (F64, 2 * B, False)}


def picture_env(ctx):
    def make():
        env = np.zeros(C_PIC * TOTAL)
        ctx.filterbank_envelope_fused(wave(), _lib.WAVE_I16, OFFS, coefs(C_PIC), B, C_PIC, True, 50.0, _lib.FFT_F32, env, None, HOST)
        return env
    return once("picture_env", make)


def picture_call(ctx, pool=0):
    def make(ctx, h, a, mem):
        ctx.check(ctx.lib.f2_envelope_picture(ctx.handle, P(a["env"]), P(OFFS), B, C_PIC, None, WIDTH, pool, P(a["pooled"]), P(a["levels"]),
                                              P(a["range"]), mem))
        return ()
    return Call({"env": picture_env(ctx)}, PIC_OUT, make)


def gtg_call(pool=0):
    def make(ctx, h, a, mem):
        ctx.check(ctx.lib.f2_gammatonegram_batch(ctx.handle, P(a["wave"]), _lib.WAVE_I16, P(OFFS), P(coefs(C_PIC)), B, C_PIC, 1, 50.0,
                                                 _lib.FFT_F32, None, WIDTH, pool, P(a["pooled"]), P(a["levels"]), P(a["range"]), mem))
        return ()
    return Call({"wave": wave()}, PIC_OUT, make)


def utterance_call():
    w = wave()[OFFS[1]:OFFS[2]].copy()

    def make(ctx, h, a, mem):
        nb = ctx.eval_utterance(h, a["wave"], _lib.WAVE_I16, len(w), coefs(C_NET), C_NET, True, 50.0, _lib.FFT_F32, RADIUS, STEP, a["env"],
                                a["scores"], a["labels"], mem)
        return (np.int64(nb),)
    return Call({"wave": w}, {"env": (F64, C_NET * len(w), True), "scores": (F32, 2 * N_UTT, True), "labels": (U8, N_UTT, True)}, make)


def strided_call(hop=HOP):
    n = sum(_lib.strided_window_count(x, RADIUS, STEP, hop) for x in LENS)

    def make(ctx, h, a, mem):
        ctx.check(ctx.lib.f2_eval_batch_strided(ctx.handle, h, P(a["wave"]), _lib.WAVE_I16, P(OFFS), P(coefs(C_NET)), B, C_NET, 1, 50.0,
                                                _lib.FFT_F32, RADIUS, STEP, hop, P(a["scores"]), P(a["labels"]), P(a["window_offsets"]), mem))
        return ()
    return Call({"wave": wave()}, {"scores": (F32, 2 * n, True), "labels": (U8, n, True), "window_offsets": (I64, B + 1, False)}, make)


CALLS = {"f2_eval_noise_sweep": lambda ctx: sweep_call(), "f2_cnn_score_windows": lambda ctx: score_call(),
         "f2_envelope_picture": picture_call, "f2_gammatonegram_batch": lambda ctx: gtg_call(),
         "f2_eval_utterance": lambda ctx: utterance_call(), "f2_eval_batch_strided": lambda ctx: strided_call()}


# ---- 1. optional outputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CALLS))
def test_optional_outputs_do_not_change_the_others(ctx, net, name):
    """All optional outputs, none, and each one alone, in host and in device memory: whatever is present equals the all-outputs
    host call bit for bit, and the mandatory results are the same in every variant."""
    call = CALLS[name](ctx)
    every = set(call.outputs)
    ref, ref_extra = call.run(ctx, net, HOST, every)
    assert all(a.size for a in ref.values())
    assert any(np.any(a) for a in ref.values())
    for mem in (HOST, DEV):
        for present in [every, set()] + [{k} for k in call.outputs]:
            got, extra = call.run(ctx, net, mem, present)
            assert set(got) == present
            for k in present:
                assert same_bits(got[k], ref[k]), (name, "device" if mem == DEV else "host", sorted(present), k)
            assert len(extra) == len(ref_extra) and all(same_bits(x, y) for x, y in zip(extra, ref_extra)), (name, mem, sorted(present))


# ---- 2. chunk boundary ---------------------------------------------------------------------------------------------------------------
N_CHUNKS = 16384 + 70


def on_device(ctx, arrays, outs, call):
    """call(pointers of arrays + outs) with everything in one arena; returns the downloaded outs"""
    with Arena(ctx) as a:
        for i, x in enumerate(arrays):
            a.region(f"in{i}", x.dtype, x.size, role="in")
        for i, (dt, n) in enumerate(outs):
            a.region(f"out{i}", dt, n, role="out")
        for i, x in enumerate(arrays):
            a.upload(f"in{i}", x)
        extra = call(*[a.ptr(f"in{i}") for i in range(len(arrays))], *[a.ptr(f"out{i}") for i in range(len(outs))])
        ctx.synchronize()
        a.check()
        return [a.download(f"out{i}") for i in range(len(outs))], extra


def test_a_host_call_of_two_chunks_equals_the_device_call(ctx, net):
    """16384 + 70 windows: the host call stages them in two chunks, the device call takes them whole. Inputs in [0, 1) (every
    chunk has the bound 1, so both calls run on the same scales): scores and labels identical. With the second chunk x 2^6 the
    host call leaves the largest chunk bound, 64, in last_input_bound."""
    n = N_CHUNKS
    x = np.random.default_rng(40).random((n, R, C_NET)).astype(F32)
    sc, lb = np.zeros(2 * n, F32), np.zeros(n, U8)
    ctx.cnn_forward(net, x, n, sc, lb, HOST)
    assert ctx.cnn_info(net, "last_input_bound") == 1.0
    (dsc, dlb), _ = on_device(ctx, [x], [(F32, 2 * n), (U8, n)], lambda dx, ds, dl: ctx.cnn_forward(net, dx, n, ds, dl, DEV))
    assert same_bits(sc, dsc) and same_bits(lb, dlb)
    assert len(np.unique(sc[2 * 16384:])) > 70      # (the second chunk came back too, and its windows were told apart)

    signs, groups = (np.arange(n) % 2).astype(U8), (np.arange(n) % GROUPS).astype(I32)
    w = x + F32(0.5)      # (strictly positive, as normalisation demands)
    for normalize, windows in ((0, x), (1, w)):
        sc, lb = np.zeros(2 * n, F32), np.zeros(n, U8)
        counts, loss = ctx.cnn_score_windows(net, windows, n, normalize, signs, groups, GROUPS, sc, lb, HOST)
        (dsc, dlb), (dcounts, dloss) = on_device(ctx, [windows, signs, groups], [(F32, 2 * n), (U8, n)], lambda dw, dsg, dg, ds, dl:
                                                 ctx.cnn_score_windows(net, dw, n, normalize, dsg, dg, GROUPS, ds, dl, DEV))
        assert same_bits(sc, dsc) and same_bits(lb, dlb) and same_bits(counts, dcounts) and same_bits(loss, dloss), normalize
        assert counts.sum() == n

    x2 = x.copy()
    x2[16384:] *= F32(64)
    ctx.cnn_forward(net, x2, n, sc, lb, HOST)
    assert ctx.cnn_info(net, "last_input_bound") == 64.0
    ctx.cnn_score_windows(net, x2, n, 0, signs, groups, GROUPS, sc, lb, HOST)
    assert ctx.cnn_info(net, "last_input_bound") == 64.0


# ---- 3. different calls back to back on one context ----------------------------------------------------------------------------------
def accuracy_call(labels):
    """f2_label_accuracy of the sweep's labels against three reference sets (utterance u against set u % 3)"""
    wo = np.zeros(U + 1, I64)
    wo[1:] = np.cumsum([_lib.strided_window_count(n, RADIUS, STEP, HOP) for n in LENS] * (K + 1))
    ref_offsets = np.array([0, 1, 4, 5], I64)
    ref_t = np.array([900, 850, 1200, 2000, 400], I64)
    ref_s = np.array([1, 0, 1, 0, 1], U8)

    def make(ctx, h, a, mem):
        return (ctx.label_accuracy(a["labels"], wo, ref_offsets, ref_t, ref_s, RADIUS * STEP, HOP, STEP, mem).copy(),)
    return Call({"labels": labels}, {}, make)


def resample_call(up, down):
    audio = np.random.default_rng(8).integers(-20000, 20000, (300, 2)).astype(I16)
    _, _, half_len, taps = design_resampler(down, up) if (up, down) != (1, 1) else (1, 1, 0, None)
    n_out = _lib.resampled_length(300, up, down)

    def make(ctx, h, a, mem):
        return (ctx.resample_batch(a["audio"], _lib.PCM_I16, 2, -1, np.array([0, 300], I64), 1, up, down, taps, half_len, a["out"], mem),)
    return Call({"audio": audio}, {"out": (F64, n_out, True)}, make)


def test_different_calls_back_to_back_share_the_context(ctx, net):
    """sweep -> label accuracy on its labels -> score windows -> picture -> resample -> sweep again, device memory, nothing waited
    for in between by the test: every result equals the same call on a fresh context, and the second sweep equals the first.
    (The small arrays of all five calls live in one scratch area of the context.)"""
    sweep, score, pic, rs = sweep_call(), score_call(), picture_call(ctx), resample_call(3, 2)
    fresh = {}
    ref_labels = None
    for key, call in (("sweep", sweep), ("accuracy", None), ("score", score), ("picture", pic), ("resample", rs)):
        c = _lib.Context(0)
        try:
            if call is None:
                call = accuracy_call(ref_labels)
            fresh[key] = call.run(c, model().handle(c), DEV, set(call.outputs))
            if key == "sweep":
                ref_labels = fresh[key][0]["labels"]
        finally:
            c.close()
    assert fresh["accuracy"][1][0].sum() > 0

    steps = [("sweep1.", sweep), ("score.", score), ("picture.", pic), ("resample.", rs), ("sweep2.", sweep)]
    with Arena(ctx) as arena:
        for prefix, call in steps:
            call.regions(arena, set(call.outputs), prefix)
        for prefix, call in steps:
            call.upload(arena, prefix)

        def go(prefix, call):
            view = _Prefixed(arena, prefix)
            return call.run(ctx, net, DEV, set(call.outputs), arena=view, wait=False)
        got = {"sweep1.": go("sweep1.", sweep)}
        acc = accuracy_call(ref_labels)      # (the inputs dict is not used below: the labels are the first sweep's, on the device)
        acc_counts = acc.make(ctx, net, {"labels": arena.ptr("sweep1.labels")}, DEV)
        for prefix, call in steps[1:]:
            got[prefix] = go(prefix, call)
        ctx.synchronize()
        arena.check()
        for prefix, call in steps:
            got[prefix][0].update(call.download(arena, set(call.outputs), prefix))

    def same(a, b):
        assert set(a[0]) == set(b[0])
        for k in a[0]:
            assert same_bits(a[0][k], b[0][k]), k
        assert all(same_bits(x, y) for x, y in zip(a[1], b[1]))
    same(got["sweep1."], fresh["sweep"])
    same(got["sweep2."], fresh["sweep"])
    assert same_bits(acc_counts[0], fresh["accuracy"][1][0])
    same(got["score."], fresh["score"])
    same(got["picture."], fresh["picture"])
    same(got["resample."], fresh["resample"])


class _Prefixed:
    """an arena seen through a name prefix (the regions of one step of the sequence)"""

    def __init__(self, arena, prefix):
        self.arena, self.prefix = arena, prefix

    def ptr(self, name):
        return self.arena.ptr(self.prefix + name)


# ---- 4. contexts that keep the guard's values ----------------------------------------------------------------------------------------
def test_guard_dump_contexts_come_and_go():
    """Twenty contexts, each with one fused call under spectral_min_rows = 0 and spectral_guard_dump = 1 (2 utterances of 5000
    samples, 8 channels), each reading the guard's values: all twenty the same, no error. The ABI has no call that reports free
    device memory, so this case cannot see whether a context gives the dump buffer back: that it does rests on the structure of
    the library (every scratch area of a context frees itself when the context goes), not on this test."""
    lens = [5000, 5000]
    w = np.concatenate([orc.synth_utterance(60 + i, n) for i, n in enumerate(lens)])
    offs = np.array([0, 5000, 10000], I64)
    first = None
    for _ in range(20):
        c = _lib.Context(0)
        try:
            c.set_option("spectral_min_rows", 0)
            c.set_option("spectral_guard_dump", 1)
            env = np.zeros(C_PIC * 10000)
            c.filterbank_envelope_fused(w, _lib.WAVE_I16, offs, coefs(C_PIC), 2, C_PIC, True, 50.0, _lib.FFT_F32, env, None, HOST)
            g = c.spectral_guard_values()
        finally:
            c.close()
        assert g.shape == (2 * C_PIC, 4)
        if first is None:
            first = (g, env)
        assert same_bits(g, first[0]) and same_bits(env, first[1])
