"""The catalogue and the sequence runner of tests/test_gpu_call_history.py.

The property under test: a call's outputs are a function of its arguments, never of the calls that came before it on the same
f2_ctx. A *call* here is a named, fully specified invocation of one entry point (fixed arguments, seeded inputs, outputs
pre-filled so that an element left unwritten shows); `call.run(ctx)` returns the raw bytes of every output plus the integer
read-backs that belong to the call.

    fresh(call)                 the call's result on a context of its own, made for it and closed after it - computed once per
                                process, and held against the independent reference of the entry point's own test file at that
                                file's tolerance before anything is compared with it (two wrong results that agree would pass
                                otherwise)
    replay(ctx, calls)          the calls one after the other on ONE context, each compared with its fresh result on raw bytes
    replay_enqueued(pairs)      the same with caller device buffers (tests/devmem.py arenas) and no wait between the calls: every
                                buffer is laid out first, then every call is enqueued, then the streams are waited for once

No tolerance lives in the history comparison: the entry points of the catalogue are the ones whose results the suite already
holds bit for bit across calls and placements (tests/test_gpu_device_placement.py `same_bits`, the "second call" assertions of the
level tests and the sweeps).

A HIP runtime error (F2_ERR_HIP) ends the pytest session: after a device fault nothing more is started on that device."""
import contextlib
import functools

import numpy as np
import pytest

import f2cnn_oracle as orc
from devmem import Arena
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel

FILL = 0x5A
HOST, DEV = _lib.MEM_HOST, _lib.MEM_DEVICE
F32, F64 = _lib.FFT_F32, _lib.FFT_F64
RADIUS, STEP = 5, 160
R = 2 * RADIUS + 1
ROUTES = {"spectral": dict(spectral=1, spectral_min_rows=0), "two_kernel": dict(spectral=0)}
TOL, TOL_F64FFT, TOL_GFB = 1e-5, 1e-10, 1e-9        # envelopes (float FFT / float64 FFT) and filterbank rows against the oracle


# ---- contexts -------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def stop_on_gpu_fault():
    try:
        yield
    except _lib.F2Error as e:
        if e.code == _lib.F2_ERR_HIP:
            pytest.exit(f"the HIP runtime reported an error ({e}): nothing more is started on this device", returncode=3)
        raise


@contextlib.contextmanager
def context():
    """A context of the caller's own; the networks made on it (network_on) go with it"""
    ctx = _lib.Context(0)
    try:
        yield ctx
    finally:
        for h in ctx.__dict__.pop("_history_networks", {}).values():
            try:
                ctx.cnn_destroy(h)
            except _lib.F2Error:
                pass
        ctx.close()


@functools.lru_cache(maxsize=None)
def model(rows, channels):
    return F2CNNModel.glorot(7, rows, channels, zero_bias=False)


def network_on(ctx, rows, channels):
    """the f2_cnn handle of model(rows, channels) on this context (F2CNNModel.handle keys its handles on id(ctx), which a later
    context may reuse)"""
    table = ctx.__dict__.setdefault("_history_networks", {})
    if (rows, channels) not in table:
        table[(rows, channels)] = ctx.cnn_create(model(rows, channels).ordered(), rows, channels)
    return table[(rows, channels)]


# ---- inputs: seeded, shared, never written to --------------------------------------------------------------------------------------
def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def wave(seed, n):
    return frozen(orc.synth_utterance(seed, n))


@functools.lru_cache(maxsize=None)
def late_click(n, before_end=5):
    """silence and one full-scale sample `before_end` samples before the end (tests/test_gpu_spectral.py: the accuracy guard sends
    such a row back to the two-kernel route inside the same call)"""
    w = np.zeros(n, np.int16)
    w[n - before_end] = 32767
    return frozen(w)


@functools.lru_cache(maxsize=None)
def table(kind, C):
    """(C, 10) coefficient tables that differ in the ways a cache key has to notice:
    erb100 / erb1000      make_erb_filters banks from 100 Hz / 1000 Hz up (ringing of the slowest channel: 256 / 64 padding samples)
    erb1000_row           erb1000 with one channel's row moved to another centre frequency
    general               A2 != 0 and B0 != 1 (tests/test_gpu_filterbank.py::test_general_coefficient_tables): never on the spectral route"""
    if kind in ("erb100", "erb1000"):
        return frozen(filters.make_erb_filters(16000, filters.centre_freqs(16000, C, int(kind[3:]))))
    if kind == "erb1000_row":
        cfs = np.array(filters.centre_freqs(16000, C, 1000), dtype=np.float64)
        cfs[C // 2] *= 1.07
        return frozen(filters.make_erb_filters(16000, cfs))
    if kind == "general":
        rng = np.random.default_rng(C + 4001)
        coefs = np.array(table("erb100", C))
        coefs[:, 5] = coefs[:, 0] * rng.uniform(-0.5, 0.5, C)
        coefs[:, 6:9] *= rng.uniform(0.5, 2.0, C)[:, None]
        return frozen(coefs)
    raise ValueError(kind)


def offsets_of(lens):
    return frozen(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))


def filled(dtype, count):
    a = np.empty(int(count), dtype)
    a.view(np.uint8)[...] = FILL
    return a


def unwritten(a):
    """elements that still hold the pre-fill of a host-memory call"""
    return int((a.view(f"u{a.dtype.itemsize}") == filled(a.dtype, 1).view(f"u{a.dtype.itemsize}")[0]).sum())


def chan_relerr(a, b):
    """per-row max |a - b| / max |b| (rows = channels), the project's envelope norm"""
    return float((np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max())


def blocks(flat, off, C):
    return [flat[C * off[b]:C * off[b + 1]].reshape(C, -1) for b in range(len(off) - 1)]


# ---- a call ----------------------------------------------------------------------------------------------------------------------
class Call:
    """name        what a failing sequence prints
    ins         {name: array} the inputs that live in the call's memory space
    outs        {name: (dtype, count)} its outputs there
    invoke      invoke(ctx, p, mem) -> {name: host array or int}: the call itself, p[name] a NumPy array (host memory) or a device
                pointer; what it returns is complete once the stream is idle
    anchor      anchor(result as arrays) raises AssertionError where the fresh result leaves its independent reference
    opts        context options held around the call
    readback    read-only integer options read after the call (they belong to its result)
    may_hold_fill   outputs whose values may equal the pre-fill by right (uint8 picture levels)"""

    def __init__(self, name, ins, outs, invoke, anchor, opts=None, readback=(), may_hold_fill=()):
        self.name, self.ins, self.outs, self.invoke, self.anchor = name, ins, outs, invoke, anchor
        self.opts, self.readback, self.may_hold_fill = dict(opts or {}), tuple(readback), tuple(may_hold_fill)
        self.dtypes = {k: np.dtype(dt) for k, (dt, _) in outs.items()}

    def __repr__(self):
        return self.name

    def _pack(self, outs, extras):
        result = {}
        for k, v in list(outs.items()) + list(extras.items()):
            a = np.ascontiguousarray(v)
            if a.dtype.kind in "iub" and k not in self.outs:
                a = a.astype(np.int64)
            self.dtypes[k] = a.dtype
            result[k] = a.tobytes()
        return result

    def arrays(self, result):
        return {k: np.frombuffer(v, self.dtypes[k]) for k, v in result.items()}

    def run(self, ctx):
        """the call in host memory: {name: raw bytes} of every output, every returned array and every read-back"""
        bufs = {k: filled(dt, n) for k, (dt, n) in self.outs.items()}
        with stop_on_gpu_fault(), ctx.options(**self.opts):
            extras = dict(self.invoke(ctx, {**self.ins, **bufs}, HOST))
            for k in self.readback:
                extras[k] = int(ctx.get_option(k))
        for k, a in bufs.items():
            if k not in self.may_hold_fill:
                assert unwritten(a) == 0, f"{self.name}: {unwritten(a)} elements of '{k}' were never written"
        return self._pack(bufs, extras)

    def prepare(self, ctx):
        """the call's buffers in ONE device allocation of the caller's, between guard bands (tests/devmem.py)"""
        return Enqueued(self, ctx)


class Enqueued:
    def __init__(self, call, ctx):
        self.call, self.ctx, self.extras = call, ctx, None
        self.arena = Arena(ctx)
        for k, a in call.ins.items():
            self.arena.region(k, a.dtype, a.size, role="in")
        for k, (dt, n) in call.outs.items():
            self.arena.region(k, dt, n, role="out")
        with stop_on_gpu_fault():
            for k, a in call.ins.items():
                self.arena.upload(k, a)
            self.p = {k: self.arena.ptr(k) for k in list(call.ins) + list(call.outs)}

    def launch(self):
        """enqueues the call; nothing waits"""
        with stop_on_gpu_fault(), self.ctx.options(**self.call.opts):
            self.extras = dict(self.call.invoke(self.ctx, self.p, DEV))

    def collect(self):
        """after the stream has been waited for: guards and inputs as they were, every output written, {name: raw bytes}"""
        try:
            with stop_on_gpu_fault():
                self.ctx.synchronize()
                self.arena.check()
                outs = {}
                for k in self.call.outs:
                    if k not in self.call.may_hold_fill:
                        assert self.arena.unwritten(k) == 0, f"{self.call.name}: elements of '{k}' were never written"
                    outs[k] = self.arena.download(k)
            return self.call._pack(outs, self.extras)
        finally:
            self.arena.free()


# ---- fresh results and sequences -----------------------------------------------------------------------------------------------------
_fresh = {}
_registry = {}


def register(call):
    """one Call per name: a second builder call with the same arguments returns the first object"""
    return _registry.setdefault(call.name, call)


def fresh(call):
    """The call's result on a context made for it, anchored; computed once"""
    if call.name not in _fresh:
        with context() as ctx:
            result = call.run(ctx)
        call.anchor(call.arrays(result))
        _fresh[call.name] = result
    return _fresh[call.name]


def differences(call, got, want):
    """[] or one line per entry whose bytes differ"""
    out = []
    for k in sorted(set(got) | set(want)):
        if k not in got or k not in want:
            if k in call.readback and k in want:
                continue                                   # (read-backs are not taken between enqueued calls)
            out.append(f"'{k}' is in one result only")
        elif got[k] != want[k]:
            a, b = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
            if len(a) != len(b):
                out.append(f"'{k}': {len(a)} bytes, fresh {len(b)}")
            else:
                bad = np.flatnonzero(a != b)
                size = call.dtypes[k].itemsize
                out.append(f"'{k}': {len(np.unique(bad // size))} of {len(a) // size} elements differ, the first at element {bad[0] // size}")
    return out


def assert_same(call, got, position, history):
    diff = differences(call, got, fresh(call))
    assert not diff, (f"call {position} of the sequence, {call.name}, is not its fresh result: " + "; ".join(diff)
                      + "\nsequence: " + " -> ".join(c.name for c in history))


def replay(ctx, calls):
    """the calls in host memory, one after the other on `ctx`, each bit for bit its fresh result"""
    calls = list(calls)
    for c in calls:
        fresh(c)                            # (references first: a failing anchor names the call, not the sequence)
    for i, c in enumerate(calls):
        assert_same(c, c.run(ctx), i, calls[:i + 1])


def replay_in_arenas(ctx, calls):
    """as replay, with caller device buffers between guard bands, waited for and checked after every call"""
    calls = list(calls)
    for c in calls:
        fresh(c)
    for i, c in enumerate(calls):
        e = c.prepare(ctx)
        e.launch()
        assert_same(c, e.collect(), i, calls[:i + 1])


def replay_enqueued(pairs):
    """pairs: [(ctx, call)]. Every buffer is laid out and uploaded first; then the calls are enqueued in order, each on its
    context's stream, with nothing waiting in between; then every stream is waited for and every result compared"""
    pairs = list(pairs)
    for _, c in pairs:
        fresh(c)
    queued = [c.prepare(ctx) for ctx, c in pairs]
    try:
        for e in queued:
            e.launch()
        results = [e.collect() for e in queued]
    finally:
        for e in queued:
            e.arena.free()
    for i, ((_, c), got) in enumerate(zip(pairs, results)):
        assert_same(c, got, i, [c for _, c in pairs[:i + 1]])


# ---- builders: filterbank, envelope, fused ---------------------------------------------------------------------------------------------
def _waves(lens, seed, f64):
    ws = [wave(7000 + 31 * seed + i, n) for i, n in enumerate(lens)]
    return [w.astype(np.float64) * 0.37 for w in ws] if f64 else ws


def filterbank(lens, C=5, tab="erb100", mode="plain", f64=False, seed=0):
    """f2_erb_filterbank_batch; mode: plain / split (k1_split = 3) / queue (k1_queue = 1) / auto (the library's own policy)"""
    opts = {"plain": dict(k1_split=0, k1_queue=0), "split": dict(k1_split=3), "queue": dict(k1_split=0, k1_queue=1), "auto": {}}[mode]
    lens = tuple(lens)
    waves, coefs, off = _waves(lens, seed, f64), table(tab, C), offsets_of(lens)
    code = _lib.WAVE_F64 if f64 else _lib.WAVE_I16

    def invoke(ctx, p, mem):
        ctx.erb_filterbank_batch(p["wave"], code, off, coefs, len(lens), C, p["gfb"], mem)
        return {}

    def anchor(r):
        for w, g in zip(waves, blocks(r["gfb"], off, C)):
            assert chan_relerr(g, orc.erb_filterbank(w, coefs)) <= TOL_GFB, len(w)
    return register(Call(f"filterbank[{mode},{tab},C{C},{'f64' if f64 else 'i16'},{list(lens)},s{seed}]",
                         {"wave": frozen(np.concatenate(waves))}, {"gfb": (np.float64, C * int(off[-1]))}, invoke, anchor, opts))


ENV_SCALE = np.array([[1.0], [3000.0], [1e-3], [1.0]])


def envelope(lens, C=4, lpf=True, cutoff=50.0, precision=F32, env_pair=1, seed=0):
    """f2_envelope_batch on seeded matrices whose rows differ in scale by six decades"""
    lens = tuple(lens)
    rng = np.random.default_rng(1000 * seed + sum(lens))
    mats = [rng.standard_normal((C, n)) * ENV_SCALE[:C] for n in lens]
    off = offsets_of(lens)

    def invoke(ctx, p, mem):
        ctx.envelope_batch(p["gfb"], off, len(lens), C, lpf, cutoff if lpf else 0.0, precision, p["env"], mem)
        return {}

    def anchor(r):
        tol = TOL if precision == F32 else TOL_F64FFT
        for m, g in zip(mats, blocks(r["env"], off, C)):
            assert chan_relerr(g, orc.extract_envelope_from_matrix(m, lpf, cutoff)) <= tol, m.shape
    name = f"envelope[{'f32' if precision == F32 else 'f64'}fft,{list(lens)},C{C},lpf {cutoff if lpf else 'off'},pair{env_pair},s{seed}]"
    return register(Call(name, {"gfb": frozen(np.concatenate([m.reshape(-1) for m in mats]))}, {"env": (np.float64, C * int(off[-1]))},
                         invoke, anchor, dict(env_pair=env_pair)))


def fused(lens, C=5, tab="erb100", lpf=True, cutoff=50.0, precision=F32, f64=False, gfb=False, route="spectral", seed=0, waves=None,
          tag="", routed=None, flagged=None, **opts):
    """f2_filterbank_envelope_fused. waves: the utterances themselves in place of the seeded ones (`tag` then names them);
    routed / flagged: what the read-backs of the fresh call must say"""
    if waves is None:
        lens = tuple(lens)
        waves = _waves(lens, seed, f64)
    else:
        lens = tuple(len(w) for w in waves)
    coefs, off = table(tab, C), offsets_of(lens)
    code = _lib.WAVE_F64 if waves[0].dtype == np.float64 else _lib.WAVE_I16

    def invoke(ctx, p, mem):
        ctx.filterbank_envelope_fused(p["wave"], code, off, coefs, len(lens), C, lpf, cutoff if lpf else 0.0, precision, p["env"],
                                      p.get("gfb"), mem)
        return {}

    def anchor(r):
        tol = TOL if precision == F32 else TOL_F64FFT
        for b, w in enumerate(waves):
            assert chan_relerr(blocks(r["env"], off, C)[b], orc.filter_and_envelope(w, coefs, lpf, cutoff)) <= tol, (b, len(w))
            if gfb:
                assert chan_relerr(blocks(r["gfb"], off, C)[b], orc.erb_filterbank(w, coefs)) <= TOL_GFB, (b, len(w))
        if routed is not None:
            assert int(r["spectral_routed"][0]) == routed, (int(r["spectral_routed"][0]), routed)
        if flagged is not None:
            assert int(r["spectral_flagged"][0]) == flagged, (int(r["spectral_flagged"][0]), flagged)
    outs = {"env": (np.float64, C * int(off[-1]))}
    if gfb:
        outs["gfb"] = (np.float64, C * int(off[-1]))
    name = (f"fused[{route},{tab},C{C},{'f64' if code == _lib.WAVE_F64 else 'i16'},{tag or list(lens)},lpf {cutoff if lpf else 'off'},"
            f"{'f32' if precision == F32 else 'f64'}fft{',gfb' if gfb else ''},s{seed}{''.join(f',{k}={v}' for k, v in sorted(opts.items()))}]")
    return register(Call(name, {"wave": frozen(np.concatenate(waves))}, outs, invoke, anchor, dict(ROUTES[route], **opts),
                         readback=("spectral_routed", "spectral_flagged")))


# ---- builders: windows, network, evaluation -----------------------------------------------------------------------------------------------
def gather_windows(C=5, N=2000, n_windows=40, seed=0):
    """f2_gather_windows at given centres, not normalised: NumPy fancy indexing cast to float32, bit for bit"""
    rng = np.random.default_rng(300 + seed)
    env = frozen(rng.random((C, N)) * 40 + 1e-3)
    centres = frozen(rng.integers(RADIUS * STEP, N - RADIUS * STEP, n_windows).astype(np.int64))

    def invoke(ctx, p, mem):
        ctx.gather_windows(p["env"], C, N, centres, n_windows, RADIUS, STEP, False, p["out"], mem)
        return {}

    def anchor(r):
        want = env[:, centres[:, None] + STEP * (np.arange(R) - RADIUS)[None, :]].transpose(1, 2, 0).astype(np.float32)
        assert r["out"].tobytes() == np.ascontiguousarray(want).tobytes()
    return register(Call(f"gather_windows[C{C},N{N},{n_windows} windows,s{seed}]", {"env": frozen(env.reshape(-1))},
                         {"out": (np.float32, n_windows * R * C)}, invoke, anchor))


def input_batch(C=5, lens=(4000, 1700, 5001), seed=0):
    """f2_input_batch; the middle utterance has no centres (tests/test_gpu_device_placement.py::test_input_batch)"""
    reach = RADIUS * STEP
    waves, coefs, off = _waves(lens, 40 + seed, False), table("erb100", C), offsets_of(lens)
    cs = [np.array([reach, 2000, lens[0] - 1 - reach], np.int64), np.zeros(0, np.int64),
          np.array([reach, 4200, 2501, lens[2] - 1 - reach], np.int64)]
    coff, centres = offsets_of([len(c) for c in cs]), frozen(np.concatenate(cs))
    nwin = int(coff[-1])

    def invoke(ctx, p, mem):
        ctx.input_batch(p["wave"], _lib.WAVE_I16, off, coefs, len(lens), C, True, 50.0, F32, coff, centres, RADIUS, STEP, False,
                        p["windows"], mem)
        return {}

    def anchor(r):
        got = r["windows"].reshape(nwin, R, C)
        for b, w in enumerate(waves):
            want = orc.gather_windows(orc.filter_and_envelope(w, coefs, True, 50), cs[b], RADIUS, STEP)
            for e in range(len(cs[b])):
                assert chan_relerr(got[coff[b] + e].T, want[e].T) <= TOL, (b, e)
    return register(Call(f"input_batch[C{C},{list(lens)},s{seed}]", {"wave": frozen(np.concatenate(waves))},
                         {"windows": (np.float32, nwin * R * C)}, invoke, anchor))


def assert_scores(scores, labels, want):
    """the bars of tests/test_gpu_device_placement.py: scores within 2e-5 of the oracle, labels the oracle's wherever its margin is clear"""
    np.testing.assert_allclose(scores, want, rtol=0, atol=2e-5)
    decided = np.abs(want[:, 1] - want[:, 0]) > 1e-4
    np.testing.assert_array_equal(labels[decided], orc.labels_from_scores(want)[decided])
    np.testing.assert_array_equal(labels, (scores[:, 1] > scores[:, 0]).astype(np.uint8))


def cnn_forward(rows=11, channels=128, n=50, scale=1.0, seed=0):
    """f2_cnn_forward on windows in [0, scale): the split path keeps one set of scales per input bound"""
    x = frozen(np.random.default_rng(3 + seed).random((n, rows, channels)).astype(np.float32) * np.float32(scale))

    def invoke(ctx, p, mem):
        h = network_on(ctx, rows, channels)
        ctx.cnn_forward(h, p["x"], n, p["scores"], p["labels"], mem)
        return {}

    def anchor(r):
        assert_scores(r["scores"].reshape(n, 2), r["labels"], orc.cnn_forward(x, dict(model(rows, channels).tensors)))
    return register(Call(f"cnn_forward[{rows}x{channels},{n} windows,x{scale:g},s{seed}]", {"x": frozen(x.reshape(-1))},
                         {"scores": (np.float32, 2 * n), "labels": (np.uint8, n)}, invoke, anchor))


EVAL_C = 40


def _window_scores(env, n, hop):
    """the oracle's scores for the windows of one utterance's envelope at the strided centres"""
    centres = (RADIUS * STEP + hop * np.arange(n)).astype(np.int64)
    w = orc.gather_windows(env, centres, RADIUS, STEP)
    return orc.cnn_forward(np.stack([orc.normalize_input(m) for m in w]), dict(model(R, EVAL_C).tensors))


def eval_batch_strided(lens=(5000, 2500), hop=160, seed=0):
    """f2_eval_batch_strided with the float64 FFT (its envelopes are the oracle's to 1e-10, so the scores are comparable at the
    forward pass's own bar, tests/test_gpu_device_placement.py::assert_eval_against_oracle)"""
    lens = tuple(lens)
    waves, coefs, off = _waves(lens, 60 + seed, False), table("erb100", EVAL_C), offsets_of(lens)
    counts = [_lib.strided_window_count(n, RADIUS, STEP, hop) for n in lens]
    nwin = sum(counts)

    def invoke(ctx, p, mem):
        h = network_on(ctx, R, EVAL_C)
        wo = ctx.eval_batch_strided(h, p["wave"], _lib.WAVE_I16, off, coefs, len(lens), EVAL_C, True, 50.0, F64, RADIUS, STEP, hop,
                                    p["scores"], p["labels"], mem)
        return {"window_offsets": wo}

    def anchor(r):
        assert r["window_offsets"].tolist() == offsets_of(counts).tolist()
        want = [_window_scores(orc.filter_and_envelope(w, coefs, True, 50), n, hop) for w, n in zip(waves, counts) if n]
        assert_scores(r["scores"].reshape(nwin, 2), r["labels"], np.concatenate(want))
    return register(Call(f"eval_batch_strided[C{EVAL_C},{list(lens)},hop {hop},s{seed}]", {"wave": frozen(np.concatenate(waves))},
                         {"scores": (np.float32, 2 * nwin), "labels": (np.uint8, nwin)}, invoke, anchor))


def eval_cutoff_sweep(lens=(2500, 3001), cutoffs=(5.0, 20.0, 50.0, 100.0, 400.0), hop=160, seed=0):
    """f2_eval_cutoff_sweep: the levels against the oracle at the envelope bar; every level's scores against the oracle's network on
    the windows of that level; the tally against counts made from the labels (tests/test_gpu_cutoff_sweep.py)"""
    lens, K, B = tuple(lens), len(cutoffs), len(lens)
    waves, coefs, off = _waves(lens, 80 + seed, False), table("erb100", EVAL_C), offsets_of(lens)
    total = int(off[-1])
    counts = [_lib.strided_window_count(n, RADIUS, STEP, hop) for n in lens]
    nwin = (K + 1) * sum(counts)

    def invoke(ctx, p, mem):
        h = network_on(ctx, R, EVAL_C)
        wo, stats = ctx.eval_cutoff_sweep(h, p["wave"], _lib.WAVE_I16, off, coefs, B, EVAL_C, F32, RADIUS, STEP, hop, cutoffs, p["env"],
                                          p["scores"], p["labels"], mem)
        return {"window_offsets": wo, "stats": stats}

    def anchor(r):
        wo, labels, scores = r["window_offsets"], r["labels"], r["scores"].reshape(nwin, 2)
        assert wo.tolist() == offsets_of(counts * (K + 1)).tolist()
        levels = r["env"].reshape(K + 1, EVAL_C * total)
        want_stats = np.zeros(((K + 1) * B, 2), np.int64)
        for l in range(K + 1):
            for b, (w, env) in enumerate(zip(waves, blocks(levels[l], off, EVAL_C))):
                ref = orc.filter_and_envelope(w, coefs, l < K, cutoffs[l] if l < K else 50)
                assert chan_relerr(env, ref) <= TOL, (l, b)
                u = l * B + b
                mine, clean = labels[wo[u]:wo[u + 1]], labels[wo[K * B + b]:wo[K * B + b + 1]]
                want_stats[u] = mine.sum(), (mine == clean).sum()
                assert_scores(scores[wo[u]:wo[u + 1]], mine, _window_scores(env, counts[b], hop))
        assert r["stats"].reshape(-1, 2).tolist() == want_stats.tolist()
    outs = {"env": (np.float64, (K + 1) * EVAL_C * total), "scores": (np.float32, 2 * nwin), "labels": (np.uint8, nwin)}
    return register(Call(f"eval_cutoff_sweep[C{EVAL_C},{list(lens)},K{K},hop {hop},s{seed}]", {"wave": frozen(np.concatenate(waves))}, outs,
                         invoke, anchor))


def gammatonegram(lens=(3000, 5001), C=5, width=64, pool=0, lpf=50, seed=0):
    """f2_gammatonegram_batch: pooled pixels against the oracle's pooled envelopes at the envelope bar, the range and the LogNorm
    levels from the device's own pooled values (tests/test_gpu_gammatonegram.py)"""
    from f2cnn_amd.scripts.plotting import PlottingProcessing as pp
    lens, B = tuple(lens), len(lens)
    waves, coefs, off = _waves(lens, 90 + seed, False), table("erb100", C), offsets_of(lens)

    def invoke(ctx, p, mem):
        rng_out = ctx.gammatonegram_batch(p["wave"], _lib.WAVE_I16, off, coefs, B, C, bool(lpf), float(lpf), F32, None, width, pool,
                                          p["pooled"], p["levels"], mem)
        return {"range": rng_out}

    def anchor(r):
        from test_gpu_gammatonegram import check_levels, positive_range
        pooled, levels, rng_out = r["pooled"].reshape(B, C, width), r["levels"].reshape(B, C, width), r["range"].reshape(B, 2)
        for b, w in enumerate(waves):
            env = orc.filter_and_envelope(w, coefs, LPF=bool(lpf), CUTOFF=lpf or 100)
            lo, hi = pp.column_edges(len(w), width)
            ref = np.array([[env[c, lo[x]:hi[x]].max() if pool else env[c, lo[x]:hi[x]].mean() for x in range(width)] for c in range(C)])
            assert (np.abs(pooled[b] - ref).max(axis=1) / env.max(axis=1)).max() <= TOL, b
            assert tuple(rng_out[b]) == positive_range(pooled[b])
        check_levels(levels, pooled, rng_out)
    outs = {"pooled": (np.float64, B * C * width), "levels": (np.uint8, B * C * width)}
    return register(Call(f"gammatonegram[C{C},{list(lens)},W{width},pool{pool},lpf{lpf},s{seed}]", {"wave": frozen(np.concatenate(waves))},
                         outs, invoke, anchor, may_hold_fill=("levels",)))


# ---- builders: levels, resampling --------------------------------------------------------------------------------------------------------
def lowpass_levels(lens=(63, 4097, 1), C=3, cutoffs=(0.5, 50.0), seed=0):
    """f2_lowpass_levels: rows against orc.low_pass_filter within 1e-12 of max |x| (the derived bound of tests/test_gpu_lowpass_levels.py),
    the copy level bit for bit"""
    lens, K = tuple(lens), len(cutoffs)
    off = offsets_of(lens)
    env = frozen(np.random.default_rng(500 + seed).standard_normal(C * int(off[-1])))

    def invoke(ctx, p, mem):
        ctx.lowpass_levels(p["env"], off, len(lens), C, cutoffs, p["levels"], mem)
        return {}

    def anchor(r):
        levels = r["levels"].reshape(K + 1, env.size)
        assert levels[K].tobytes() == env.tobytes()
        for l, cutoff in enumerate(cutoffs):
            for x, y in zip(blocks(env, off, C), blocks(levels[l], off, C)):
                for c in range(C):
                    assert np.abs(y[c] - orc.low_pass_filter(x[c], cutoff)).max() <= 1e-12 * np.abs(x[c]).max(), (l, c, x.shape)
    return register(Call(f"lowpass_levels[C{C},{list(lens)},{list(cutoffs)},s{seed}]", {"env": env}, {"levels": (np.float64, (K + 1) * env.size)},
                         invoke, anchor))


def reverb_levels(lens=(1, 1025, 2085), taps=(2, 1025), seed=0):
    """f2_reverb_levels on int16 samples and integer taps in [-8, 8]: every partial sum is an integer below 2^53, so
    numpy.convolve(x, h)[:n] is the result in any order of the sum, bit for bit (tests/test_gpu_reverb_levels.py)"""
    lens, K = tuple(lens), len(taps)
    rng = np.random.default_rng(600 + seed)
    off = offsets_of(lens)
    x = frozen(rng.integers(-32768, 32768, int(off[-1])).astype(np.int16))
    rirs = [rng.integers(-8, 9, t).astype(np.float64) for t in taps]
    for h in rirs:
        h[0] = h[0] or 1.0

    def invoke(ctx, p, mem):
        ctx.reverb_levels(p["wave"], _lib.WAVE_I16, off, len(lens), rirs, p["levels"], mem)
        return {}

    def anchor(r):
        levels = r["levels"].reshape(K + 1, len(x))
        assert levels[K].tobytes() == x.astype(np.float64).tobytes()
        for l, h in enumerate(rirs):
            for b in range(len(lens)):
                xb = x[off[b]:off[b + 1]].astype(np.float64)
                assert levels[l, off[b]:off[b + 1]].tobytes() == (np.convolve(xb, h)[:len(xb)] + 0.0).tobytes(), (l, b)
    return register(Call(f"reverb_levels[{list(lens)},taps {list(taps)},s{seed}]", {"wave": x}, {"levels": (np.float64, (K + 1) * len(x))},
                         invoke, anchor))


def channel_mix_levels(lens=(3, 513, 1), C=5, K=2, seed=0):
    """f2_channel_mix_levels on integer envelopes and integer weights in [-8, 8]: the matrix product bit for bit in any order of the
    sum (tests/test_gpu_channel_mix_levels.py)"""
    lens = tuple(lens)
    rng = np.random.default_rng(700 + seed)
    off = offsets_of(lens)
    env = frozen(rng.integers(-32768, 32768, C * int(off[-1])).astype(np.float64))
    mix = frozen(rng.integers(-8, 9, (K, C, C)).astype(np.float64))

    def invoke(ctx, p, mem):
        ctx.channel_mix_levels(p["env"], off, len(lens), C, mix, p["levels"], mem)
        return {}

    def anchor(r):
        levels = r["levels"].reshape(K + 1, env.size)
        assert levels[K].tobytes() == env.tobytes()
        for l in range(K):
            for src, got in zip(blocks(env, off, C), blocks(levels[l], off, C)):
                assert got.tobytes() == np.ascontiguousarray(mix[l] @ src + 0.0).tobytes(), l
    return register(Call(f"channel_mix_levels[C{C},{list(lens)},K{K},s{seed}]", {"env": env}, {"levels": (np.float64, (K + 1) * env.size)},
                         invoke, anchor))


def resample(up=160, down=441, beta=5.0, lens=(1500, 2, 701), seed=0):
    """f2_resample_batch with resample_poly's taps for a Kaiser window of `beta` (5: scipy's default filter), held against
    resample_poly inside the rounding bound of two dot products of T + 1 operations (tests/test_gpu_resample.py)"""
    from scipy.signal import firwin, resample_poly
    lens = tuple(lens)
    half_len = 10 * max(up, down)
    window = firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", beta))
    taps = frozen(window * up)
    off = offsets_of(lens)
    x = frozen(np.random.default_rng(800 + seed).integers(-32768, 32768, int(off[-1])).astype(np.int16))
    want_off = offsets_of([_lib.resampled_length(n, up, down) for n in lens])

    def invoke(ctx, p, mem):
        oo = ctx.resample_batch(p["audio"], _lib.PCM_I16, 1, -1, off, len(lens), up, down, taps, half_len, p["out"], mem)
        return {"out_offsets": oo}

    def anchor(r):
        assert r["out_offsets"].tolist() == want_off.tolist()
        T = -(-(2 * half_len + 1) // up)
        padded = np.zeros(T * up)
        padded[:2 * half_len + 1] = np.abs(taps)
        g = (T + 1) * 2.0 ** -53 / (1.0 - (T + 1) * 2.0 ** -53)
        bound = 2.0 * g * float(np.abs(x.astype(np.float64)).max()) * padded.reshape(T, up).sum(axis=0).max()
        for b in range(len(lens)):
            ref = resample_poly(x[off[b]:off[b + 1]].astype(np.float64), up, down, window=window)
            got = r["out"][want_off[b]:want_off[b + 1]]
            assert got.shape == ref.shape and np.abs(got - ref).max() <= bound, b
    return register(Call(f"resample[{up}/{down},kaiser {beta:g},{list(lens)},s{seed}]", {"audio": x}, {"out": (np.float64, int(want_off[-1]))},
                         invoke, anchor))


# ---- the catalogue -----------------------------------------------------------------------------------------------------------------------------
def catalogue():
    """Every entry point of the list in the module text of tests/test_gpu_call_history.py at the smallest shapes that reach its code
    paths: C of 4 or 5 (65: a second channel group), the shortest row of each length class, tens of windows. {name: Call}"""
    calls = [
        filterbank((1599, 33, 1, 4099)), filterbank((1599, 33, 4099), mode="split"), filterbank((1599, 33, 1, 4099), mode="queue"),
        filterbank((1599, 33, 4099), tab="general"), filterbank((1599, 300), C=65), filterbank((1599, 33), f64=True),
        envelope((3, 1000, 4097)), envelope((8193,)), envelope((16385,)), envelope((32769,), env_pair=1), envelope((32769,), env_pair=0),
        envelope((65537,), C=2), envelope((3, 1000, 4097), precision=F64), envelope((8193,), precision=F64, lpf=False),
        fused((4097, 300, 8193)), fused((4097, 300, 8193), route="two_kernel"), fused((16385, 32769), C=4),
        fused((4097, 300), f64=True), fused((4097, 300), f64=True, route="two_kernel"),
        fused((4097, 300), gfb=True), fused((4097, 300), gfb=True, route="two_kernel"), fused((1599, 4099), C=65),
        gather_windows(), input_batch(), cnn_forward(11, 128), cnn_forward(13, 40), eval_batch_strided(),
        lowpass_levels(), reverb_levels(), channel_mix_levels(), resample(), eval_cutoff_sweep(), gammatonegram(),
    ]
    return {c.name: c for c in calls}
