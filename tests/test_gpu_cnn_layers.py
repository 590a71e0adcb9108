"""f2_cnn_layers: conv4's pooled output and dense1's output of every route of the CNN forward pass, element by element against the
float64 referee (tests/cnn_layers_referee.py, which states the measure and where the tolerances come from), at the shapes where the
kernels change tile counts, branches or routes - and the entry's own promises: a forced route runs its kernels or refuses, route
"call" is f2_cnn_forward, outputs are optional and the same bytes in both memory spaces.

Measured on an MI355X, worst e_w over all shapes and both input kinds (the float32 CPU chain has 6.7e-7; TOL32 = 2.68e-6, the split
layers get twice that): float32 kernels and recorded forward 1.32e-6 pooled / 1.81e-6 dense1, per-tile split kernels 1.29e-6 /
1.58e-6, weight-stationary kernels 6.5e-7 / 1.49e-6 with either dense1; scores within 7.3e-8. Per shape: DESIGN.md, "K4 per element".
13 x 76 x 9, the one shape with a second x-tile in the layer-by-layer float32 kernels: float32 kernels and recorded forward 8.5e-7 /
6.0e-7, per-tile split route (float32 conv3 / conv4) 6.7e-7 / 1.45e-6, scores within 5.0e-8; the float32 CPU chain 3.0e-7 / 3.5e-7.
"""
import numpy as np
import pytest

import cnn_layers_referee as lr
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

FORCED = ("f32", "tile", "ws", "ws_dense")


def case_id(c):
    return "{}x{}x{}".format(*c)


def routes_of(case):
    return (FORCED if case in lr.WS_CASES else FORCED[:2]) + ("recorded",)


RUNS = [(c, r) for c in lr.WS_CASES + lr.OFF_WS_CASES for r in routes_of(c)]
RUN_IDS = ["{}-{}".format(case_id(c), r) for c, r in RUNS]
BIG_RUNS = [(c, r) for c in lr.BIG_CASES for r in routes_of(c)]
BIG_IDS = ["{}-{}".format(case_id(c), r) for c, r in BIG_RUNS]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def tolerances(case, route):
    """(pooled, dense1): TOL32 where the float32 kernels made the layer - conv3 / conv4 of the mixed route included -, else twice that"""
    if route in ("f32", "recorded"):       # (the recorded forward of the gradient chain is float32 throughout)
        return lr.TOL32, lr.TOL32
    return (lr.TOL_SPLIT if lr.dims(case[0], case[1]).Hp1 == 4 else lr.TOL32), lr.TOL_SPLIT


def capable(ctx, model, route):
    """asserts that f2_cnn_create's self-check left the kernels of `route` on for this network: no run below can pass by falling back"""
    h = model.handle(ctx)
    assert ctx.cnn_info(h, "f16x3_ok") == 1
    if route in ("ws", "ws_dense") or (model.rows, model.channels) in [c[:2] for c in lr.WS_CASES]:
        assert ctx.cnn_info(h, "ws_ok") == 1 and ctx.cnn_info(h, "ws_dense_ok") == 1 and ctx.cnn_info(h, "f16x3_ok") == 1


_ran = {}


def device(ctx, case, kind, route):
    """(pooled, dense1, scores) of the device for the referee's windows on a forced route, computed once per module"""
    key = (id(ctx), case, kind, route)
    if key not in _ran:
        ref = lr.referee(*case, kind)
        capable(ctx, ref.model, route)
        out = ref.model.layers(ref.x, route, ctx=ctx)
        for a in out:
            a.setflags(write=False)
        _ran[key] = out
    return _ran[key]


def against_float64(ctx, case, kind, route):
    ref = lr.referee(*case, kind)
    pooled, dense1, scores = device(ctx, case, kind, route)
    assert pooled.dtype == dense1.dtype == scores.dtype == np.float32
    tol_p, tol_d = tolerances(case, route)
    what = "{} {} {}".format(case_id(case), kind, route)
    print("float32 CPU chain {}: pooled {:.3g}, dense1 {:.3g}".format(what, lr.window_errors(ref.pooled32, ref.pooled64).max(),
                                                                       lr.window_errors(ref.dense32, ref.dense64).max()))
    lr.check("pooled", pooled, ref.pooled64, tol_p, case[0], case[1], what)
    lr.check("dense1", dense1, ref.dense64, tol_d, case[0], case[1], what)
    err = np.abs(scores.astype(np.float64) - ref.scores64).max()
    print("{} scores: max |device - float64| {:.3g}".format(what, err))
    assert err <= 2e-5, what


@pytest.mark.parametrize("case,route", RUNS, ids=RUN_IDS)
def test_pooled_and_dense1_against_float64(ctx, case, route):
    against_float64(ctx, case, "unit", route)


@pytest.mark.parametrize("case,route", RUNS, ids=RUN_IDS)
def test_dense1_alone(ctx, case, route):
    """dense1 of the device against dense1 recomputed in float64 from the pooled array the device itself returned: a fault here is
    dense1's (kernel or weight packing), whatever the convolutions did"""
    ref = lr.referee(*case, "unit")
    pooled, dense1, _ = device(ctx, case, "unit", route)
    lr.check("dense1", dense1, lr.dense1_of(pooled, ref.model), tolerances(case, route)[1], case[0], case[1],
             "{} {} from the device's pooled".format(case_id(case), route))


@pytest.mark.parametrize("case,route", BIG_RUNS, ids=BIG_IDS)
def test_inputs_beyond_one(ctx, case, route):
    """windows times 2^10: the scale sets of B = 2^10, and the input scale and conv1 tap scale of k_conv12_ws. The tolerances are
    relative to each window's maximum, so they are the ones of inputs in [0, 1)."""
    ref = lr.referee(*case, "big")
    ref.model.predict(ref.x, ctx=ctx)
    assert ctx.cnn_info(ref.model.handle(ctx), "last_input_bound") == 1024.0     # the split path took these windows, with that set
    against_float64(ctx, case, "big", route)
    pooled, dense1, _ = device(ctx, case, "big", route)
    lr.check("dense1", dense1, lr.dense1_of(pooled, ref.model), tolerances(case, route)[1], case[0], case[1],
             "{} big {} from the device's pooled".format(case_id(case), route))


@pytest.mark.parametrize("case", lr.OFF_WS_CASES, ids=case_id)
def test_shapes_off_the_weight_stationary_route_refuse_it(ctx, case):
    ref = lr.referee(*case, "unit")
    h = ref.model.handle(ctx)
    assert ctx.cnn_info(h, "ws_ok") == 0 and ctx.cnn_info(h, "ws_dense_ok") == 0 and ctx.cnn_info(h, "f16x3_ok") == 1
    for route in ("ws", "ws_dense"):
        with pytest.raises(_lib.F2Error) as e:
            ref.model.layers(ref.x, route, ctx=ctx)
        assert e.value.code == _lib.F2_ERR_UNSUPPORTED, route


def test_call_route_is_f2_cnn_forward(ctx):
    case = (11, 128, 193)
    ref = lr.referee(*case, "unit")
    m = ref.model
    capable(ctx, m, "ws_dense")
    keys = ("cnn_f16x3", "cnn_ws", "cnn_ws_dense")
    assert [ctx.get_option(k) for k in keys] == [1, 1, 1]
    call = m.layers(ref.x, "call", ctx=ctx)
    assert call[2].tobytes() == m.predict(ref.x, ctx=ctx).tobytes()
    forced = device(ctx, case, "unit", "ws_dense")
    assert call[0].tobytes() == forced[0].tobytes() and call[1].tobytes() == forced[1].tobytes() and call[2].tobytes() == forced[2].tobytes()
    f32 = device(ctx, case, "unit", "f32")
    assert call[0].tobytes() != f32[0].tobytes() and call[1].tobytes() != f32[1].tobytes()         # (the routes are not one)
    ws = device(ctx, case, "unit", "ws")
    assert ws[0].tobytes() == forced[0].tobytes()                  # the same convolutions ...
    print("dense1 of k_dense1_ws and of the per-tile kernel differ in {} of {} elements, by at most {:.3g}".format(
        int((ws[1] != forced[1]).sum()), ws[1].size, float(np.abs(ws[1] - forced[1]).max())))
    try:
        for k in keys:
            ctx.set_option(k, 0)
        call0 = m.layers(ref.x, "call", ctx=ctx)
        assert call0[2].tobytes() == m.predict(ref.x, ctx=ctx).tobytes()
        for a, b in zip(call0, f32):
            assert a.tobytes() == b.tobytes()
        # a forced route ignores the options
        again = m.layers(ref.x, "ws_dense", ctx=ctx)
        for a, b in zip(again, forced):
            assert a.tobytes() == b.tobytes()
    finally:
        for k in keys:
            ctx.set_option(k, 1)


def test_recorded_route_is_the_gradient_chains_forward(ctx):
    """its scores are f2_cnn_input_gradient's, and a call of more than one chunk of the chain (1024 windows) gives every window the
    bits it has in a call of its own"""
    case = (10, 18, 33)
    ref = lr.referee(*case, "unit")
    m = ref.model
    assert device(ctx, case, "unit", "recorded")[2].tobytes() == m.input_gradient(ref.x, ctx=ctx)[1].tobytes()
    x = np.random.default_rng(5).random((1100, case[0], case[1])).astype(np.float32)
    whole = m.layers(x, "recorded", ctx=ctx)
    tail = m.layers(x[1000:], "recorded", ctx=ctx)
    for a, b in zip(whole, tail):
        assert a[1000:].tobytes() == b.tobytes()
    assert whole[2].tobytes() == m.input_gradient(x, ctx=ctx)[1].tobytes()
    f32 = m.layers(x, "f32", ctx=ctx)
    assert np.abs(whole[2] - f32[2]).max() <= 5e-7


@pytest.mark.parametrize("case", lr.WS_CASES + lr.OFF_WS_CASES, ids=case_id)
def test_recorded_route_has_the_float32_routes_bits(ctx, case):
    """Other kernels, the same sums: conv1 is an fmaf chain in tap order on both routes, conv2 .. conv4 run the one 9-tap loop of
    f2_cnn_f32_tile.h (conv_taps) whether fused or layer by layer, bias + ReLU commute with the max of the pool, and dense1 is
    the same kernel. So pooled, dense1 and scores are the same bytes."""
    recorded, f32 = device(ctx, case, "unit", "recorded"), device(ctx, case, "unit", "f32")
    for name, a, b in zip(("pooled", "dense1", "scores"), recorded, f32):
        assert a.tobytes() == b.tobytes(), "{} {}: {} of {} elements differ".format(case_id(case), name, int((a != b).sum()), a.size)


def layers_raw(ctx, model, x, n, route, mem, want=(True, True, True), x_arg="x"):
    """f2_cnn_layers through the bare binding with -7.0-filled outputs in memory space `mem`: ([pooled, dense1, scores] or None
    where not asked, error code or 0)"""
    flat = lr.dims(model.rows, model.channels).flat
    rows = min(max(int(n), 1), len(x))      # (a refused call writes nothing: no need for the rows it names)
    out = [np.full((rows, w), -7.0, np.float32) if on else None for w, on in zip((flat, 516, 2), want)]
    h = model.handle(ctx)
    code = 0
    if mem != _lib.MEM_DEVICE:
        try:
            ctx.cnn_layers(h, x if x_arg == "x" else None, n, route, out[0], out[1], out[2], mem)
        except _lib.F2Error as e:
            code = e.code
        return out, code
    d_x = ctx.malloc(x.nbytes)
    d_out = [ctx.malloc(a.nbytes) if a is not None else None for a in out]
    try:
        ctx.h2d(d_x, x)
        for d, a in zip(d_out, out):
            if a is not None:
                ctx.h2d(d, a)
        try:
            ctx.cnn_layers(h, d_x if x_arg == "x" else None, n, route, d_out[0], d_out[1], d_out[2], mem)
        except _lib.F2Error as e:
            code = e.code
        ctx.synchronize()
        for d, a in zip(d_out, out):
            if a is not None:
                ctx.d2h(a, d)
    finally:
        for d in [d_x] + d_out:
            if d is not None:
                ctx.free(d)
    return out, code


@pytest.mark.parametrize("case,route", [((11, 18, 97), "ws_dense"), ((13, 40, 33), "tile"), ((18, 20, 33), "f32"), ((14, 24, 33), "recorded")],
                         ids=lambda v: case_id(v) if isinstance(v, tuple) else v)
def test_outputs_optional_memory_spaces_and_errors(ctx, case, route):
    ref = lr.referee(*case, "unit")
    m, x, n = ref.model, ref.x, case[2]
    R = _lib.CNN_ROUTES
    capable(ctx, m, route)
    full, code = layers_raw(ctx, m, x, n, R[route], _lib.MEM_HOST)
    assert code == 0
    for a, b in zip(full, device(ctx, case, "unit", route)):
        assert a.tobytes() == b.tobytes()
    dev, code = layers_raw(ctx, m, x, n, R[route], _lib.MEM_DEVICE)
    assert code == 0
    for a, b in zip(dev, full):
        assert a.tobytes() == b.tobytes()
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for k in range(3):
            want = tuple(j == k for j in range(3))
            one, code = layers_raw(ctx, m, x, n, R[route], mem, want)
            assert code == 0 and one[k].tobytes() == full[k].tobytes(), (mem, k)
        none, code = layers_raw(ctx, m, x, n, R[route], mem, (False, False, False))
        assert code == 0
        # argument errors and refusals write nothing
        nan = x.copy()
        nan[n // 2, 1, 1] = np.nan
        refused = [(x, n, 9, "x", _lib.F2_ERR_INVALID), (x, n, -1, "x", _lib.F2_ERR_INVALID), (x, -1, R[route], "x", _lib.F2_ERR_INVALID),
                   (x, n, R[route], None, _lib.F2_ERR_INVALID), (x, 16385, R[route], "x", _lib.F2_ERR_UNSUPPORTED)]
        if route in FORCED[1:]:
            refused.append((nan, n, R[route], "x", _lib.F2_ERR_UNSUPPORTED))
        if case in lr.OFF_WS_CASES:
            refused += [(x, n, R["ws"], "x", _lib.F2_ERR_UNSUPPORTED), (x, n, R["ws_dense"], "x", _lib.F2_ERR_UNSUPPORTED)]
        for xx, nn, rr, xa, want_code in refused:
            out, code = layers_raw(ctx, m, xx, nn, rr, mem, x_arg=xa)
            assert code == want_code, (mem, nn, rr, xa, code)
            assert all((a == -7.0).all() for a in out), (mem, nn, rr, xa)
        out, code = layers_raw(ctx, m, x, n, R[route], 5)
        assert code == _lib.F2_ERR_INVALID and all((a == -7.0).all() for a in out)
        out, code = layers_raw(ctx, m, x, 0, R[route], mem)
        assert code == 0 and all((a == -7.0).all() for a in out)
    # the float32 kernels take the NaN window, and it spoils no other window's bits
    got, code = layers_raw(ctx, m, nan, n, R["f32"], _lib.MEM_HOST)
    assert code == 0
    clean = m.layers(x, "f32", ctx=ctx)
    keep = np.arange(n) != n // 2
    for a, b in zip(got, clean):
        assert a[keep].tobytes() == b[keep].tobytes()
    with pytest.raises(ValueError):
        m.layers(x, "fastest", ctx=ctx)
    with pytest.raises(ValueError):
        m.layers(x[:, :-1], "f32", ctx=ctx)


@pytest.mark.parametrize("case", [(11, 70, 9), (14, 24, 9)], ids=case_id)
def test_dead_network(ctx, case):
    """zero windows through a network without biases: every activation is exactly 0 on every route, whatever its scales"""
    m = F2CNNModel.glorot(7, case[0], case[1], zero_bias=True)
    x = np.zeros((case[2], case[0], case[1]), np.float32)
    for route in routes_of((case[0], case[1], 33)) + ("call",):
        if route != "call":
            capable(ctx, m, route)
        pooled, dense1, scores = m.layers(x, route, ctx=ctx)
        assert not pooled.any() and not dense1.any(), route
        assert (scores == 0.5).all(), route
