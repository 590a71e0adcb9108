"""The eight entry points that take caller data share one host path (argument checks, wave staging, the two-kernel envelope
sequence, one eval body): f2_eval_utterance is f2_eval_batch with one utterance, bit for bit, its envelope output is the fused
call's on the two-kernel route, and every entry point refuses every bad argument it has before it launches anything."""
import ctypes

import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

C, RADIUS, STEP = 128, 5, 160
R = 2 * RADIUS + 1
# no window, one window, one CNN chunk (14 240 windows), three chunks (38 240: more than CNN_CHUNK = 16 384 windows in one
# utterance, the case whose dense layers run per group of chunks), and a row of more than 65 536 samples (four-step envelope route)
LENGTHS = (1700, 1761, 16000, 40000, 70000)


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
    return F2CNNModel.glorot(11)


class Buffers:
    """Arrays of one call in the memory space under test: numpy arrays for MEM_HOST, device allocations (freed by close) otherwise"""

    def __init__(self, ctx, mem):
        self.ctx, self.mem, self.dev = ctx, mem, []

    def put(self, arr):
        if self.mem == _lib.MEM_HOST:
            return arr
        p = self.ctx.malloc(max(arr.nbytes, 8))
        self.dev.append(p)
        self.ctx.h2d(p, arr)
        return p

    def out(self, shape, dtype):
        """an output array filled with the byte 0x5A (what the call did not write shows up), and its handle"""
        a = np.frombuffer(b"\x5a" * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()
        return a, self.put(a)

    def get(self, host, handle):
        if self.mem != _lib.MEM_HOST and host.nbytes:
            self.ctx.d2h(host, handle)
        return host

    def close(self):
        self.ctx.synchronize()
        for p in self.dev:
            self.ctx.free(p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("mem", [_lib.MEM_HOST, _lib.MEM_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("dt", [_lib.WAVE_I16, _lib.WAVE_F64], ids=["i16", "f64"])
@pytest.mark.parametrize("lpf", [False, True], ids=["nolpf", "lpf50"])
@pytest.mark.parametrize("N", LENGTHS)
def test_eval_utterance_is_eval_batch_with_one_utterance(ctx, coefs, model, N, lpf, dt, mem):
    h = model.handle(ctx)
    wave = orc.synth_utterance(100 + N % 97, N)
    if dt == _lib.WAVE_F64:
        wave = wave.astype(np.float64)
    cutoff = 50.0 if lpf else 0.0
    nb = max(N - R * STEP, 0)
    offs = np.array([0, N], np.int64)
    buf = Buffers(ctx, mem)
    try:
        w = buf.put(wave)
        env_u, p_env_u = buf.out((C, N), np.float64)
        sc_u, p_sc_u = buf.out((nb, 2), np.float32)
        lb_u, p_lb_u = buf.out((nb,), np.uint8)
        got = ctx.eval_utterance(h, w, dt, N, coefs, C, lpf, cutoff, _lib.FFT_F32, RADIUS, STEP, p_env_u, p_sc_u, p_lb_u, mem)
        ctx.synchronize()
        buf.get(env_u, p_env_u), buf.get(sc_u, p_sc_u), buf.get(lb_u, p_lb_u)
        assert got == nb

        sc_b, p_sc_b = buf.out((nb, 2), np.float32)
        lb_b, p_lb_b = buf.out((nb,), np.uint8)
        ctx.eval_batch(h, w, dt, offs, coefs, 1, C, lpf, cutoff, _lib.FFT_F32, RADIUS, STEP, p_sc_b, p_lb_b, mem)
        ctx.synchronize()
        buf.get(sc_b, p_sc_b), buf.get(lb_b, p_lb_b)
        assert np.array_equal(bits(sc_u), bits(sc_b)), f"scores differ in {np.count_nonzero((sc_u != sc_b).any(axis=1))} of {nb} windows"
        assert np.array_equal(lb_u, lb_b)
        if nb:
            assert sc_u.min() >= 0 and sc_u.max() <= 1 and set(np.unique(lb_u)) <= {0, 1}       # (written: not the fill byte)

        # the envelope output: the fused call on the two-kernel route, whatever the length
        env_f, p_env_f = buf.out((C, N), np.float64)
        with ctx.options(spectral=0):
            ctx.filterbank_envelope_fused(w, dt, offs, coefs, 1, C, lpf, cutoff, _lib.FFT_F32, p_env_f, None, mem)
        ctx.synchronize()
        buf.get(env_f, p_env_f)
        assert np.array_equal(bits(env_u), bits(env_f))
        assert np.isfinite(env_u).all() and np.abs(env_u).max() < 1e9                     # (the same)
    finally:
        buf.close()


# ---- one argument test over all eight entry points ----
LENS = (2000, 1900)
TOTAL = sum(LENS)
NWIN = 16

ORDER = {
    "f2_erb_filterbank_batch": "ctx wave wave_dtype offsets coefs B C gfb mem_space",
    "f2_envelope_batch": "ctx gfb offsets B C lpf cutoff_hz fft_precision env mem_space",
    "f2_filterbank_envelope_fused": "ctx wave wave_dtype offsets coefs B C lpf cutoff_hz fft_precision env null mem_space",
    "f2_gather_windows": "ctx env1 C N1 null n_win radius step normalize windows mem_space",
    "f2_cnn_forward": "ctx cnn x n_win scores labels mem_space",
    "f2_eval_utterance": "ctx cnn wave wave_dtype N1 coefs C lpf cutoff_hz fft_precision radius step env scores labels nb_out mem_space",
    "f2_eval_batch": "ctx cnn wave wave_dtype offsets coefs B C lpf cutoff_hz fft_precision radius step scores labels mem_space",
    "f2_input_batch": "ctx wave wave_dtype offsets coefs B C lpf cutoff_hz fft_precision center_offsets centers radius step normalize "
                      "windows mem_space",
}
PIPELINE = ("f2_gather_windows", "f2_cnn_forward", "f2_eval_utterance", "f2_eval_batch", "f2_input_batch")
# argument class -> {argument: bad value}; a call has the class when it has all of its arguments
BAD = {
    "null_ctx": {"ctx": None},
    "bad_mem_space": {"mem_space": 7},
    "bad_wave_dtype": {"wave_dtype": 5},
    "bad_fft_precision": {"fft_precision": 3},
    "lpf_cutoff_0": {"lpf": 1, "cutoff_hz": 0.0},
    "lpf_cutoff_8000": {"lpf": 1, "cutoff_hz": 8000.0},
    "lpf_cutoff_negative": {"lpf": 1, "cutoff_hz": -1.0},
    "offsets_start_not_0": {"offsets": np.array([1, LENS[0], TOTAL], np.int64)},
    "offsets_decrease": {"offsets": np.array([0, LENS[0], LENS[0] - 1], np.int64)},
    "cnn_of_another_shape": {"cnn": "cnn13", "radius": RADIUS},     # (13-row network, 11-row windows asked for)
}
CASES = [(fn, cls) for fn, names in ORDER.items() for cls, bad in BAD.items() if set(bad) <= set(names.split())]
# the memory space that only the calls of the plain filterbank / envelope family take
CASES += [(fn, "mem_host_async_not_taken") for fn in PIPELINE]


def valid_arguments(ctx, coefs, model):
    rng = np.random.default_rng(5)
    wave = np.concatenate([orc.synth_utterance(31 + i, n) for i, n in enumerate(LENS)])
    a = {
        "ctx": ctx.handle, "null": None, "mem_space": _lib.MEM_HOST, "wave": wave, "wave_dtype": _lib.WAVE_I16,
        "offsets": np.array([0, LENS[0], TOTAL], np.int64), "coefs": coefs, "B": len(LENS), "C": C, "lpf": 1, "cutoff_hz": 50.0,
        "fft_precision": _lib.FFT_F32, "gfb": rng.standard_normal((C, TOTAL)), "env": np.empty((C, TOTAL)),
        "env1": rng.random((C, LENS[0])) + 0.5, "N1": LENS[0], "n_win": NWIN, "radius": RADIUS, "step": STEP, "normalize": 1,
        "windows": np.empty((NWIN, R, C), np.float32), "x": rng.random((NWIN, R, C), dtype=np.float32),
        "scores": np.empty((TOTAL, 2), np.float32), "labels": np.empty(TOTAL, np.uint8), "nb_out": ctypes.c_int64(),
        "center_offsets": np.array([0, 2, 3], np.int64), "centers": np.array([800, 1000, 900], np.int64),
        "cnn": model.handle(ctx),
    }
    return a


def call(fn, a):
    def raw(v):
        if isinstance(v, np.ndarray):
            return v.ctypes.data
        return ctypes.byref(v) if isinstance(v, ctypes.c_int64) else v
    return getattr(_lib.load(), fn)(*[raw(a[name]) for name in ORDER[fn].split()])


@pytest.fixture(scope="module")
def cnn13(ctx):
    return F2CNNModel.glorot(11, rows=13).handle(ctx)


@pytest.mark.parametrize("fn", list(ORDER))
def test_the_valid_call_of_the_argument_test_runs(ctx, coefs, model, fn):
    """(the arguments that the next test spoils one at a time are a call that launches kernels)"""
    a = valid_arguments(ctx, coefs, model)
    ctx.prof_enable(True)
    try:
        assert call(fn, a) == _lib.F2_OK, _lib.load().f2_last_error(ctx.handle).decode()
        assert ctx.prof_get()
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("fn,cls", CASES, ids=[f"{fn}-{cls}" for fn, cls in CASES])
def test_bad_argument_is_refused_before_anything_is_launched(ctx, coefs, model, cnn13, fn, cls):
    a = valid_arguments(ctx, coefs, model)
    bad = {"mem_space": _lib.MEM_HOST_ASYNC} if cls == "mem_host_async_not_taken" else BAD[cls]
    a.update({k: (cnn13 if isinstance(v, str) else v) for k, v in bad.items()})
    ctx.prof_enable(True)
    try:
        assert call(fn, a) == _lib.F2_ERR_INVALID
        assert ctx.prof_get() == {}
    finally:
        ctx.prof_enable(False)
