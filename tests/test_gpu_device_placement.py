"""The F2_MEM_DEVICE contract of include/f2cnn_hip.h, held at placements a caller's tensor slice produces: every buffer inside
somebody else's allocation (tests/devmem.py: one arena, guard bands of poison on both sides of every region) and starting an odd
number of elements past a 256-byte boundary. Every case runs the same call at the reference placement (every region on a
boundary) and at an odd one, and asserts

  1. at the reference placement, agreement with the oracle at the bar the project already holds that entry point to;
  2. the outputs at the odd placement are bit-identical to the reference placement's. No kernel here forms a sum in an order
     that depends on the address: placement changes which store schedule runs (f2_filterbank.hip `lagged`, the vector / scalar
     body of f2_cnn_range.hip, whose maximum has no order), not the arithmetic - so no case uses a looser bar;
  3. arena.check(): every guard band and every input byte for byte as before the call (an `inout` region excepted);
  4. no element of an output still holds its pre-fill.

Misalignments are in elements of the buffer's own type: float64 1 / 5 / 15 (8, 40, 120 bytes: 120 is the last slot of a
128-byte line, a 16-byte pair store there straddles two lines), float32 1 / 3 / 31, int16 1 / 3, uint8 1 / 3.

What the kernels do to caller-supplied pointers (widest access, alignment it relies on), read from f2cnn_amd/csrc before the
first run of this file. Global memory of gfx950 takes wide accesses at any dword-aligned address, so none of these asks for more
than the header grants:

  wave     int16 / float64   one element per load (f2_filterbank.hip, f2_spectral.hip k_utterance_spectrum / k_tail_state,
                             f2_noise.hip): element alignment
  gfb out  float64           one element per store; the store lag of a row comes from the absolute address (`phase_c0`)
  gfb in   float64           16-byte pair loads through f2_d2u, declared aligned(8) (f2_envelope_core.h); element loads elsewhere
  env out  float64           16-byte pair stores through f2_d2u (aligned(8)); the spectral kernels store 16 / 8 bytes through a
                             buffer descriptor of exactly the row (base 8-byte aligned, offsets multiples of 8, range-checked);
                             parked intermediates - 4-byte buffer accesses (long spectral rows) and 8-byte float pairs (on-chip
                             2-4 s kernel) - lie inside the row they belong to
  env in   float64           one element per load (f2_gather.hip)
  windows / out  float32     one element per store; the blocked every-sample kernel stores float4 when C % 4 == 0 through a
                             type that claims 16-byte alignment where only 4 is given (f2_gather.hip eval_windows_body): the
                             instruction is the same global_store_dwordx4 an aligned(4) type compiles to, and C = 8 at out
                             misalign 1 / 3 / 31 runs it
  x        float32           k_conv12_ws: global_load_lds_dword, one dword per lane; per-tile conv1: one element per load;
                             range pass: float4 loads only when ((uintptr_t)x & 15) == 0, else one element
  windows in (score), scores, labels, signs, groups   one element per access (4, 4, 1, 1, 4 bytes)
"""
import numpy as np
import pytest

import f2cnn_oracle as orc
import label_referee as lr
from conftest import chan_relerr
from devmem import Arena, ArenaViolation
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

I16, F64, F32, U8, I32 = np.int16, np.float64, np.float32, np.uint8, np.int32
RADIUS, STEP, R = 5, 160, 11
REACH = RADIUS * STEP
DEV = _lib.MEM_DEVICE


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def erb_coefs(C):
    return filters.make_erb_filters(16000, filters.centre_freqs(16000, C, 100))


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def placed(ctx, bufs, mis, call):
    """One call at one placement. bufs: {name: (dtype, count, role, data or None)}; mis: {name: misalign}, 0 where not named;
    call(pointers) makes the call and may return something (host outputs). Asserts 3. and 4. of the module text; returns
    ({name: array} of the out / inout regions, what `call` returned)."""
    assert set(mis) <= set(bufs), (set(mis), set(bufs))
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
            if role != "in":
                outs[name] = a.download(name)
        return outs, extra


_cache = {}


def once(key, make):
    """references and reference-placement results: computed once per key, shared, never written to"""
    def freeze(v):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, (tuple, list, dict)):
            for a in (v.values() if isinstance(v, dict) else v):
                freeze(a)
    if key not in _cache:
        _cache[key] = make()
        freeze(_cache[key])
    return _cache[key]


def blocks(flat, off, C):
    """the (C, n_b) matrices of a ragged (C * total) output"""
    return [flat[C * off[b]:C * off[b + 1]].reshape(C, -1) for b in range(len(off) - 1)]


# ---- K1: f2_erb_filterbank_batch -------------------------------------------------------------------------------------------------
K1_LENS = [1599, 33, 1, 4099, 0, 2050]
K1_OPTS = {"plain": dict(k1_split=0, k1_queue=0), "split": dict(k1_split=3), "queue": dict(k1_split=0, k1_queue=1)}
# (wave type, wave misalign, gfb misalign)
K1_PLACES = [("i16", 1, 1), ("i16", 3, 5), ("f64", 1, 15)]


def k1_batch(wtype):
    waves = [orc.synth_utterance(300 + i, n) for i, n in enumerate(K1_LENS)]
    if wtype == "f64":
        waves = [w.astype(F64) * 0.37 for w in waves]
    return waves


def general_table(C):
    """A2 != 0 and B0 != 1, as tests/test_gpu_filterbank.py::test_general_coefficient_tables builds it"""
    rng = np.random.default_rng(C + 4001)
    coefs = erb_coefs(C).copy()
    coefs[:, 5] = coefs[:, 0] * rng.uniform(-0.5, 0.5, C)
    coefs[:, 6:9] *= rng.uniform(0.5, 2.0, C)[:, None]
    return coefs


def k1_run(ctx, waves, coefs, C, opts, mis, short_by=0):
    off = offsets_of([len(w) for w in waves])
    flat = np.concatenate(waves)
    wdt, wcode = (I16, _lib.WAVE_I16) if flat.dtype == np.int16 else (F64, _lib.WAVE_F64)
    bufs = {"wave": (wdt, len(flat), "in", flat), "gfb": (F64, C * int(off[-1]) - short_by, "out", None)}

    def call(p):
        with ctx.options(**opts):
            ctx.erb_filterbank_batch(p["wave"], wcode, off, coefs, len(waves), C, p["gfb"], DEV)
    return placed(ctx, bufs, mis, call)[0]["gfb"], off


@pytest.mark.parametrize("wtype,wmis,gmis", K1_PLACES)
@pytest.mark.parametrize("mode", list(K1_OPTS))
@pytest.mark.parametrize("C", [5, 65])
def test_filterbank(ctx, C, mode, wtype, wmis, gmis):
    """C = 65: a second wave group of one row, so the kernel's `full_rows` is false there. A non-zero base phase gives row 0 of
    utterance 0 a store lag, which an allocation-aligned output never does."""
    coefs, waves = erb_coefs(C), k1_batch(wtype)
    ref, off = once(("k1", C, mode, wtype), lambda: k1_run(ctx, waves, coefs, C, K1_OPTS[mode], {}))
    want = once(("k1_oracle", C, wtype), lambda: [orc.erb_filterbank(w, coefs) for w in waves])
    for g, o in zip(blocks(ref, off, C), want):
        assert g.shape == o.shape
        if g.size:
            assert chan_relerr(g, o) <= 1e-9
    got, _ = k1_run(ctx, waves, coefs, C, K1_OPTS[mode], {"wave": wmis, "gfb": gmis})
    assert same_bits(got, ref)


@pytest.mark.parametrize("wtype,wmis,gmis", K1_PLACES)
def test_filterbank_general_coefficient_table(ctx, wtype, wmis, gmis):
    C = 5
    coefs, waves = general_table(C), k1_batch(wtype)
    ref, off = once(("k1_general", wtype), lambda: k1_run(ctx, waves, coefs, C, K1_OPTS["plain"], {}))
    for g, w in zip(blocks(ref, off, C), waves):
        if g.size:
            assert chan_relerr(g, orc.erb_filterbank(w, coefs)) <= 1e-9
    got, _ = k1_run(ctx, waves, coefs, C, K1_OPTS["plain"], {"wave": wmis, "gfb": gmis})
    assert same_bits(got, ref)


def test_the_arena_sees_a_kernels_write_past_a_region(ctx):
    """The detector fires on a real kernel: the gfb region is declared one element SHORTER than the call's output (the element
    lies in the region's tail guard, inside the allocation), so the filterbank's last store is a write exactly 0 bytes past the
    region's end."""
    coefs, waves = erb_coefs(5), k1_batch("i16")
    with pytest.raises(ArenaViolation) as e:
        k1_run(ctx, waves, coefs, 5, K1_OPTS["plain"], {"wave": 1, "gfb": 1}, short_by=1)
    assert (e.value.region, e.value.where, e.value.distance) == ("gfb", "after", 0), str(e.value)
    assert e.value.changed <= 8


# ---- K2: f2_envelope_batch ---------------------------------------------------------------------------------------------------------
K2_SCALE = np.array([[1.0], [3000.0], [1e-3]])
# name: (lengths, C, options, FFT precisions)
K2_BATCHES = {
    "short": ([3, 1000, 4097], 3, {}, (_lib.FFT_F32, _lib.FFT_F64)),
    "n16001": ([16001], 3, {}, (_lib.FFT_F32, _lib.FFT_F64)),
    "on_chip": ([32769, 40000], 3, dict(env_pair=1), (_lib.FFT_F32,)),
    "four_step": ([32769, 40000], 3, dict(env_pair=0), (_lib.FFT_F32,)),
    "n70001": ([70001], 3, {}, (_lib.FFT_F32,)),
    "n262145": ([262145], 2, {}, (_lib.FFT_F32,)),
}
K2_CASES = [(name, p) for name, v in K2_BATCHES.items() for p in v[3]]
# out of place: gfb at 1, env at 15; in place: one inout region at 1 and at 15
K2_PLACES = {"apart": dict(gfb=1, env=15), "inplace1": dict(io=1), "inplace15": dict(io=15)}


def k2_mats(name):
    lens, C = K2_BATCHES[name][:2]
    rng = np.random.default_rng(sum(lens))
    return [rng.standard_normal((C, n)) * K2_SCALE[:C] for n in lens]


def k2_run(ctx, name, lpf, precision, inplace, mis):
    lens, C, opts, _ = K2_BATCHES[name]
    off = offsets_of(lens)
    flat = once(("k2_in", name), lambda: np.concatenate([m.reshape(-1) for m in k2_mats(name)]))
    if inplace:
        bufs = {"io": (F64, len(flat), "inout", flat)}
    else:
        bufs = {"gfb": (F64, len(flat), "in", flat), "env": (F64, len(flat), "out", None)}

    def call(p):
        with ctx.options(**opts):
            ctx.envelope_batch(p["io" if inplace else "gfb"], off, len(lens), C, lpf, 50.0 if lpf else 0.0, precision,
                               p["io" if inplace else "env"], DEV)
    return placed(ctx, bufs, mis, call)[0]["io" if inplace else "env"]


@pytest.mark.parametrize("lpf", [False, True], ids=["magnitude", "lpf50"])
@pytest.mark.parametrize("place", list(K2_PLACES))
@pytest.mark.parametrize("name,precision", K2_CASES)
def test_envelope(ctx, name, precision, place, lpf):
    lens, C = K2_BATCHES[name][:2]
    off, inplace = offsets_of(lens), place != "apart"
    tol = 1e-5 if precision == _lib.FFT_F32 else 1e-10
    ref = once(("k2", name, precision, inplace, lpf), lambda: k2_run(ctx, name, lpf, precision, inplace, {}))
    want = once(("k2_oracle", name, lpf), lambda: [orc.extract_envelope_from_matrix(m, lpf, 50) for m in k2_mats(name)])
    for g, o in zip(blocks(ref, off, C), want):
        assert chan_relerr(g, o) <= tol, g.shape
    assert same_bits(k2_run(ctx, name, lpf, precision, inplace, K2_PLACES[place]), ref)


# ---- f2_filterbank_envelope_fused ------------------------------------------------------------------------------------------------
FUSED_LENS = [16000, 4097, 20001, 40001, 300, 33001]
FUSED_OPTS = {"spectral": dict(spectral=1, spectral_min_rows=0), "two_kernel": dict(spectral=0)}
FUSED_PLACES = {"a": dict(wave=1, env=15, gfb=5), "b": dict(wave=3, env=1, gfb=15)}
# (lengths, C, route, gfb output, FFT precision, placement)
FUSED_CASES = [(FUSED_LENS, 5, route, gfb, _lib.FFT_F32, pl) for route in FUSED_OPTS for gfb in (False, True) for pl in FUSED_PLACES]
FUSED_CASES += [(FUSED_LENS, 5, "spectral", True, _lib.FFT_F64, "a"), ([1599, 4099], 65, "spectral", False, _lib.FFT_F32, "a")]


def fused_run(ctx, waves, coefs, C, route, want_gfb, precision, mis):
    off = offsets_of([len(w) for w in waves])
    flat = np.concatenate(waves)
    bufs = {"wave": (I16, len(flat), "in", flat), "env": (F64, C * len(flat), "out", None)}
    if want_gfb:
        bufs["gfb"] = (F64, C * len(flat), "out", None)

    def call(p):
        with ctx.options(**FUSED_OPTS[route]):
            ctx.filterbank_envelope_fused(p["wave"], _lib.WAVE_I16, off, coefs, len(waves), C, True, 50.0, precision, p["env"],
                                          p.get("gfb"), DEV)
            return ctx.get_option("spectral_routed"), ctx.get_option("spectral_flagged")
    outs, routed = placed(ctx, bufs, {k: v for k, v in mis.items() if k in bufs}, call)
    return outs, routed


@pytest.mark.parametrize("lens,C,route,want_gfb,precision,place", FUSED_CASES)
def test_fused(ctx, lens, C, route, want_gfb, precision, place):
    coefs = erb_coefs(C)
    waves = once(("fused_waves", tuple(lens)), lambda: [orc.synth_utterance(900 + i, n) for i, n in enumerate(lens)])
    off = offsets_of(lens)
    ref, routed = once(("fused", tuple(lens), C, route, want_gfb, precision),
                       lambda: fused_run(ctx, waves, coefs, C, route, want_gfb, precision, {}))
    want = once(("fused_oracle", tuple(lens), C), lambda: [orc.erb_filterbank(w, coefs) for w in waves])
    want_env = once(("fused_oracle_env", tuple(lens), C), lambda: [orc.extract_envelope_from_matrix(g, True, 50) for g in want])
    tol = 1e-5 if precision == _lib.FFT_F32 else 1e-10
    for b in range(len(lens)):
        assert chan_relerr(blocks(ref["env"], off, C)[b], want_env[b]) <= tol, b
        if want_gfb:
            assert chan_relerr(blocks(ref["gfb"], off, C)[b], want[b]) <= 1e-9, b
    if route == "spectral" and precision == _lib.FFT_F32 and not want_gfb:
        assert routed[0] >= 1                          # (the one-kernel route is under test, not only its fall-back)
    got, routed_odd = fused_run(ctx, waves, coefs, C, route, want_gfb, precision, FUSED_PLACES[place])
    assert routed_odd == routed                        # spectral_routed, spectral_flagged
    for k in ref:
        assert same_bits(got[k], ref[k]), k


# ---- K3: f2_gather_windows ---------------------------------------------------------------------------------------------------------
K3_N = 2000
K3_CENTRES = np.array([800, 1199, 801], np.int64)
K3_MODES = {"centres": None, "blocked": 1, "per_window": 0}          # every-sample normalised windows: option gather_blocked


def k3_env(C):
    return once(("k3_env", C), lambda: np.random.default_rng(C).random((C, K3_N)) * 40 + 1e-3)


def k3_run(ctx, C, mode, mis):
    env = k3_env(C)
    nwin = len(K3_CENTRES) if mode == "centres" else K3_N - R * STEP
    bufs = {"env": (F64, env.size, "in", env), "out": (F32, nwin * R * C, "out", None)}

    def call(p):
        if mode == "centres":
            ctx.gather_windows(p["env"], C, K3_N, K3_CENTRES, nwin, RADIUS, STEP, False, p["out"], DEV)
        else:
            with ctx.options(gather_blocked=K3_MODES[mode]):
                ctx.gather_windows(p["env"], C, K3_N, None, nwin, RADIUS, STEP, True, p["out"], DEV)
    return placed(ctx, bufs, mis, call)[0]["out"].reshape(nwin, R, C)


@pytest.mark.parametrize("omis", [1, 3, 31])
@pytest.mark.parametrize("mode", list(K3_MODES))
@pytest.mark.parametrize("C", [8, 7])
def test_gather_windows(ctx, C, mode, omis):
    """C = 8: the blocked kernel's 16-byte row stores (f2_gather.hip, `(C & 3) == 0`) at an address that is only 4-byte
    aligned; C = 7: its scalar rows."""
    ref = once(("k3", C, mode), lambda: k3_run(ctx, C, mode, {}))
    if mode == "centres":
        assert same_bits(ref, orc.gather_windows(k3_env(C), K3_CENTRES).astype(F32))
    else:
        assert ref.shape[0] == 240
        np.testing.assert_allclose(ref, orc.eval_input_tensor(k3_env(C))[..., 0], rtol=0, atol=2e-7)
    assert same_bits(k3_run(ctx, C, mode, {"env": 1, "out": omis}), ref)


# ---- f2_input_batch ----------------------------------------------------------------------------------------------------------------
def test_input_batch(ctx):
    """The middle utterance has no centres (and is too short for a window)."""
    C, lens = 8, [4000, 1700, 5001]
    coefs = erb_coefs(C)
    waves = [orc.synth_utterance(40 + i, n) for i, n in enumerate(lens)]
    off, flat = offsets_of(lens), np.concatenate(waves)
    cs = [np.array([REACH, 2000, 4000 - 1 - REACH], np.int64), np.zeros(0, np.int64), np.array([REACH, 4200, 2501, 5000 - REACH], np.int64)]
    coff, centres = offsets_of([len(c) for c in cs]), np.concatenate(cs)
    nwin = int(coff[-1])
    bufs = {"wave": (I16, len(flat), "in", flat), "windows": (F32, nwin * R * C, "out", None)}

    def call(p):
        ctx.input_batch(p["wave"], _lib.WAVE_I16, off, coefs, 3, C, True, 50.0, _lib.FFT_F32, coff, centres, RADIUS, STEP, False,
                        p["windows"], DEV)
    ref = placed(ctx, bufs, {}, call)[0]["windows"].reshape(nwin, R, C)
    for b, w in enumerate(waves):
        want = orc.gather_windows(orc.filter_and_envelope(w, coefs, True, 50), cs[b], RADIUS, STEP)
        for e in range(len(cs[b])):
            assert chan_relerr(ref[coff[b] + e].T, want[e].T) <= 1e-5, (b, e)       # per window, channels as rows
    got = placed(ctx, bufs, {"wave": 1, "windows": 3}, call)[0]["windows"].reshape(nwin, R, C)
    assert same_bits(got, ref)


# ---- K4: f2_cnn_forward ------------------------------------------------------------------------------------------------------------
K4_SHAPES = [(11, 128), (11, 67), (13, 40)]
K4_ROUTES = {"default": {}, "no_ws": dict(cnn_ws=0), "f32": dict(cnn_f16x3=0)}
K4_PLACES = {"a": dict(x=1, scores=1, labels=1), "b": dict(x=3, scores=1, labels=3)}
K4_N = (1, 97, 193)


def k4_model(rows, channels):
    return once(("k4_model", rows, channels), lambda: F2CNNModel.glorot(7, rows, channels, zero_bias=False))


def k4_x(rows, channels):
    return once(("k4_x", rows, channels), lambda: np.random.default_rng(3).random((max(K4_N), rows, channels)).astype(F32))


def k4_oracle(rows, channels, n):
    """the oracle treats every window on its own: windows [0, 1), [1, 97), [97, 193) are each computed once and shared"""
    edges = (0,) + K4_N
    parts = [once(("k4_oracle", rows, channels, lo), lambda: orc.cnn_forward(k4_x(rows, channels)[lo:hi],
                                                                              dict(k4_model(rows, channels).tensors)))
             for lo, hi in zip(edges, edges[1:]) if hi <= n]
    return np.concatenate(parts)


def k4_run(ctx, model, x, route, mis, scores=True, labels=True):
    n = len(x)
    bufs = {"x": (F32, x.size, "in", x)}
    if scores:
        bufs["scores"] = (F32, 2 * n, "out", None)
    if labels:
        bufs["labels"] = (U8, n, "out", None)
    h = model.handle(ctx)

    def call(p):
        with ctx.options(**K4_ROUTES[route]):
            ctx.cnn_forward(h, p["x"], n, p.get("scores"), p.get("labels"), DEV)
        return ctx.cnn_info(h, "last_input_bound")
    return placed(ctx, bufs, {k: v for k, v in mis.items() if k in bufs}, call)


@pytest.mark.parametrize("rows,channels", K4_SHAPES)
def test_cnn_models_serve_the_routes_under_test(ctx, rows, channels):
    """f2_cnn_create's self-check admits the kernels the routes below name: the split-fp16 path for every shape, the
    weight-stationary kernels for the 11-row shapes (so "default" and "no_ws" are different kernels there)."""
    h = k4_model(rows, channels).handle(ctx)
    assert ctx.cnn_info(h, "f16x3_ok") == 1
    assert ctx.cnn_info(h, "ws_ok") == ctx.cnn_info(h, "ws_dense_ok") == (1 if rows == 11 else 0)


@pytest.mark.parametrize("n", K4_N)
@pytest.mark.parametrize("place", list(K4_PLACES))
@pytest.mark.parametrize("route", list(K4_ROUTES))
@pytest.mark.parametrize("rows,channels", K4_SHAPES)
def test_cnn_forward(ctx, rows, channels, route, place, n):
    model = k4_model(rows, channels)
    x = k4_x(rows, channels)[:n]
    ref, bound = once(("k4", rows, channels, route, n), lambda: k4_run(ctx, model, x, route, {}))
    want = k4_oracle(rows, channels, n)
    scores = ref["scores"].reshape(n, 2)
    np.testing.assert_allclose(scores, want, rtol=0, atol=2e-5)
    decided = np.abs(want[:, 1] - want[:, 0]) > 1e-4
    np.testing.assert_array_equal(ref["labels"][decided], orc.labels_from_scores(want)[decided])
    np.testing.assert_array_equal(ref["labels"], (scores[:, 1] > scores[:, 0]).astype(U8))
    got, bound_odd = k4_run(ctx, model, x, route, K4_PLACES[place])
    assert bound_odd == bound == (-1 if route == "f32" else 1)
    assert same_bits(got["scores"], ref["scores"]) and same_bits(got["labels"], ref["labels"])


@pytest.mark.parametrize("scores,labels", [(False, True), (True, False)], ids=["scores_null", "labels_null"])
def test_cnn_forward_with_an_output_left_out(ctx, scores, labels):
    model, x = k4_model(11, 67), k4_x(11, 67)[:97]
    full, _ = once(("k4", 11, 67, "default", 97), lambda: k4_run(ctx, model, x, "default", {}))
    for mis in ({}, K4_PLACES["b"]):
        got, _ = k4_run(ctx, model, x, "default", mis, scores=scores, labels=labels)
        assert set(got) == {"labels" if labels else "scores"}
        for k in got:
            assert same_bits(got[k], full[k]), k


def test_cnn_forward_scaled_input_takes_the_scalar_range_pass(ctx):
    """x at misalign 1 is 4 bytes past a 16-byte boundary: f2_launch_cnn_input_range takes its scalar body there and the
    16-byte body at the reference placement; both must find the same range (inputs below 300: the bound 512)."""
    model = k4_model(11, 128)
    x = np.ascontiguousarray(k4_x(11, 128)[:97] * np.float32(300.0))
    ref, bound = k4_run(ctx, model, x, "default", {})
    np.testing.assert_allclose(ref["scores"].reshape(-1, 2), orc.cnn_forward(x, dict(model.tensors)), rtol=0, atol=2e-5)
    got, bound_odd = k4_run(ctx, model, x, "default", dict(x=1, scores=1, labels=1))
    assert bound == 512 and bound_odd == 512
    assert same_bits(got["scores"], ref["scores"]) and same_bits(got["labels"], ref["labels"])


# ---- f2_eval_utterance / f2_eval_batch / f2_eval_batch_strided ---------------------------------------------------------------------
EVAL_C = 40
EVAL_LENS = [2500, 1700, 3001]
EVAL_PLACE = dict(wave=1, scores=1, labels=3, env=5)


def eval_model():
    return once("eval_model", lambda: F2CNNModel.glorot(7, 11, EVAL_C))


def eval_waves():
    return once("eval_waves", lambda: [orc.synth_utterance(2028 + i, n) for i, n in enumerate(EVAL_LENS)])


def eval_oracle_env(b):
    return once(("eval_oracle_env", b), lambda: orc.filter_and_envelope(eval_waves()[b], erb_coefs(EVAL_C), True, 50))


EVAL_PARTS = 4


def eval_part(b, part):
    """rows [lo, hi) of utterance b's every-sample windows: the oracle's forward pass is taken a quarter at a time"""
    nb = max(0, EVAL_LENS[b] - R * STEP)
    return nb * part // EVAL_PARTS, nb * (part + 1) // EVAL_PARTS


def eval_oracle_scores(b, part):
    """the oracle's scores for those windows: what orc.eval_input_tensor builds, for the centres of this part"""
    def make():
        lo, hi = eval_part(b, part)
        w = orc.gather_windows(eval_oracle_env(b), orc.eval_window_centers(EVAL_LENS[b], RADIUS, STEP)[lo:hi], RADIUS, STEP)
        x = np.stack([orc.normalize_input(m) for m in w]) if hi > lo else np.zeros((0, R, EVAL_C))
        return orc.cnn_forward(x, dict(eval_model().tensors))
    return once(("eval_oracle_scores", b, part), make)


def eval_oracle_scores_of(b):
    return np.concatenate([eval_oracle_scores(b, part) for part in range(EVAL_PARTS)])


def assert_eval_against_oracle(scores, labels, want):
    """the K4 bars, for the float64 FFT: its envelopes are the oracle's to 1e-10, so the windows are the oracle's to the 2e-7 of
    the window test and the scores are comparable at the forward pass's own bar. (With the float FFT the logarithm of the
    quietest samples moves the windows by up to 2e-3, tests/test_gpu_input_from_wav.py, and the chain is held to 5e-4 elsewhere.)"""
    np.testing.assert_allclose(scores, want, rtol=0, atol=2e-5)
    decided = np.abs(want[:, 1] - want[:, 0]) > 1e-4
    np.testing.assert_array_equal(labels[decided], orc.labels_from_scores(want)[decided])


def eval_run(ctx, kind, hop, precision, mis):
    coefs, h = erb_coefs(EVAL_C), eval_model().handle(ctx)
    waves = eval_waves()[:1] if kind == "utterance" else eval_waves()
    lens = [len(w) for w in waves]
    off, flat = offsets_of(lens), np.concatenate(waves)
    nwin = sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in lens)
    bufs = {"wave": (I16, len(flat), "in", flat), "scores": (F32, 2 * nwin, "out", None), "labels": (U8, nwin, "out", None)}
    if kind == "utterance":
        bufs["env"] = (F64, EVAL_C * lens[0], "out", None)

    def call(p):
        args = (coefs, len(lens), EVAL_C, True, 50.0, precision, RADIUS, STEP)
        if kind == "utterance":
            return ctx.eval_utterance(h, p["wave"], _lib.WAVE_I16, lens[0], coefs, EVAL_C, True, 50.0, precision, RADIUS, STEP,
                                      p["env"], p["scores"], p["labels"], DEV)
        if kind == "batch":
            return ctx.eval_batch(h, p["wave"], _lib.WAVE_I16, off, *args, p["scores"], p["labels"], DEV)
        return ctx.eval_batch_strided(h, p["wave"], _lib.WAVE_I16, off, *args, hop, p["scores"], p["labels"], DEV).tolist()
    return placed(ctx, bufs, {k: v for k, v in mis.items() if k in bufs}, call)


@pytest.mark.parametrize("part", range(EVAL_PARTS))
@pytest.mark.parametrize("b", [0, 2])
def test_eval_batch_rows_against_the_oracle(ctx, b, part):
    """f2_eval_batch (float64 FFT) at the reference placement, a quarter of an utterance's windows per case (test_eval_calls
    holds the whole calls against the same oracle scores, shared from here)."""
    ref, _ = once(("eval", "batch", 1, _lib.FFT_F64), lambda: eval_run(ctx, "batch", 1, _lib.FFT_F64, {}))
    first = sum(max(0, n - R * STEP) for n in EVAL_LENS[:b])
    lo, hi = eval_part(b, part)
    assert hi > lo
    assert_eval_against_oracle(ref["scores"].reshape(-1, 2)[first + lo:first + hi], ref["labels"][first + lo:first + hi],
                               eval_oracle_scores(b, part))


@pytest.mark.parametrize("precision", [_lib.FFT_F32, _lib.FFT_F64], ids=["fft32", "fft64"])
@pytest.mark.parametrize("kind,hop", [("utterance", 1), ("batch", 1), ("strided", 1), ("strided", 16), ("strided", 7)])
def test_eval_calls(ctx, kind, hop, precision):
    ref, extra = once(("eval", kind, hop, precision), lambda: eval_run(ctx, kind, hop, precision, {}))
    utts = range(1 if kind == "utterance" else len(EVAL_LENS))
    scores = ref["scores"].reshape(-1, 2)
    assert len(scores) == sum(_lib.strided_window_count(EVAL_LENS[b], RADIUS, STEP, hop) for b in utts) > 0
    np.testing.assert_array_equal(ref["labels"], (scores[:, 1] > scores[:, 0]).astype(U8))
    if precision == _lib.FFT_F64:
        assert_eval_against_oracle(scores, ref["labels"], np.concatenate([eval_oracle_scores_of(b)[::hop] for b in utts]))
    if kind == "utterance":
        # env_or_null in device memory serves as the call's envelope buffer itself
        assert extra == EVAL_LENS[0] - R * STEP
        assert chan_relerr(ref["env"].reshape(EVAL_C, -1), eval_oracle_env(0)) <= 1e-5
    if kind == "strided":
        assert extra == offsets_of([_lib.strided_window_count(n, RADIUS, STEP, hop) for n in EVAL_LENS]).tolist()
    got, extra_odd = eval_run(ctx, kind, hop, precision, EVAL_PLACE)
    assert extra_odd == extra
    for k in ref:
        assert same_bits(got[k], ref[k]), k


# ---- f2_eval_noise_sweep, f2_label_accuracy, f2_cnn_score_windows: everything the header places in mem_space at misalign 1 ----------
def test_noise_sweep(ctx):
    coefs, h = erb_coefs(EVAL_C), eval_model().handle(ctx)
    waves = eval_waves()[:2]
    lens = [len(w) for w in waves]
    off, flat = offsets_of(lens), np.concatenate(waves)
    snr, hop, levels = np.array([0.0, 10.0]), 16, 3
    nwin = levels * sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in lens)
    bufs = {"wave": (I16, len(flat), "in", flat), "noisy": (F64, levels * len(flat), "out", None),
            "scores": (F32, 2 * nwin, "out", None), "labels": (U8, nwin, "out", None)}

    def call(p):
        return ctx.eval_noise_sweep(h, p["wave"], _lib.WAVE_I16, off, coefs, 2, EVAL_C, True, 50.0, _lib.FFT_F32, RADIUS, STEP, hop,
                                    snr, 77, p["noisy"], p["scores"], p["labels"], DEV)
    ref, (wo, sigma, stats) = placed(ctx, bufs, {}, call)
    assert wo[-1] == nwin > 0 and (sigma[:4] > 0).all() and (sigma[4:] == 0).all()
    assert same_bits(ref["noisy"][2 * len(flat):], flat.astype(F64))                   # the clean level
    assert np.array_equal(stats[4:, 1], np.diff(wo)[4:])
    got, (wo1, sigma1, stats1) = placed(ctx, bufs, {k: 1 for k in bufs}, call)
    assert np.array_equal(wo1, wo) and same_bits(sigma1, sigma) and np.array_equal(stats1, stats)
    for k in ref:
        assert same_bits(got[k], ref[k]), k


def test_label_accuracy(ctx):
    rng = np.random.default_rng(17)
    wo = offsets_of([301, 0, 777])
    labels = rng.integers(0, 2, int(wo[-1])).astype(U8)
    ro = offsets_of([4, 1, 5])
    T = np.array([100, 260, 500, 1700, 50, 10, 170, 900, 1000, 5000], np.int64)
    s = rng.integers(0, 2, len(T)).astype(U8)
    hop, origin = 7, REACH
    want = np.stack([lr.referee(labels[wo[u]:wo[u + 1]], T[ro[u]:ro[u + 1]], s[ro[u]:ro[u + 1]], origin, hop) for u in range(3)])
    assert want[0].sum() > 0 and want[2].sum() > 0 and want[1].sum() == 0
    bufs = {"labels": (U8, len(labels), "in", labels)}

    def call(p):
        return ctx.label_accuracy(p["labels"], wo, ro, T, s, origin, hop, STEP, DEV)
    for mis in ({}, {"labels": 1}, {"labels": 3}):
        _, counts = placed(ctx, bufs, mis, call)
        assert np.array_equal(counts, want), mis


@pytest.mark.parametrize("normalize", [1, 0])
def test_cnn_score_windows(ctx, normalize):
    n, G = 300, 3
    rng = np.random.default_rng(23)
    w = np.exp(rng.normal(0.0, 1.0, (n, R, EVAL_C))).astype(F32)
    signs, groups = rng.integers(0, 2, n).astype(U8), rng.integers(0, G, n).astype(I32)
    h = eval_model().handle(ctx)
    bufs = {"windows": (F32, w.size, "in", w), "signs": (U8, n, "in", signs), "groups": (I32, n, "in", groups),
            "scores": (F32, 2 * n, "out", None), "labels": (U8, n, "out", None)}

    def call(p):
        return ctx.cnn_score_windows(h, p["windows"], n, normalize, p["signs"], p["groups"], G, p["scores"], p["labels"], DEV)
    ref, (counts, loss) = placed(ctx, bufs, {}, call)
    want = np.zeros((G, 2, 2), np.int64)
    np.add.at(want, (groups, signs, ref["labels"].astype(np.int64)), 1)
    assert np.array_equal(counts, want) and counts.sum() == n and (loss > 0).all()
    got, (counts1, loss1) = placed(ctx, bufs, {k: 1 for k in bufs}, call)
    assert np.array_equal(counts1, counts) and same_bits(loss1, loss)
    for k in ref:
        assert same_bits(got[k], ref[k]), k
