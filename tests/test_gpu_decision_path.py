"""f2_decision_path: the smoothed decision per row against the sequential referee (tests/segments_referee.py) - path, emissions
and optimum exact at every row count around a wave, a tile and the scan's chunk, four penalties, three scales; streams made of
ties, clipped scores and NaNs; one utterance alone and in a batch, two calls, host and device memory byte for byte; device buffers
at odd element misalignment between guard bands; argument errors with the outputs untouched."""
import numpy as np
import pytest

import segments_cases as sc
import segments_referee as ref
from devmem import Arena
from f2cnn_amd import _lib

pytestmark = pytest.mark.gpu
H, D = _lib.MEM_HOST, _lib.MEM_DEVICE


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def host_call(ctx, scores, wo, scale, penalty, want_q=True):
    n = int(wo[-1])
    path = np.full(n, 7, np.uint8)
    q = np.full(n, -77, np.int32) if want_q else None
    value = ctx.decision_path(scores, wo, scale, penalty, path, H, emissions=q)
    return path, q, value


def device_call(ctx, scores, wo, scale, penalty):
    n = int(wo[-1])
    with Arena(ctx) as a:
        a.region("scores", np.float32, 2 * n, misalign=1, role="in")
        a.region("path", np.uint8, n, misalign=3, role="out")
        a.region("q", np.int32, n, misalign=1, role="out")
        a.upload("scores", scores)
        value = ctx.decision_path(a.ptr("scores"), wo, scale, penalty, a.ptr("path"), D, emissions=a.ptr("q"))
        ctx.synchronize()
        a.check()
        return a.download("path").copy(), a.download("q").copy(), value


def test_the_random_streams_stand_clear_of_half_integers():
    assert sc.clearance(sc.random_scores()) >= sc.CLEAR


@pytest.mark.parametrize("scale,penalty", sc.CASES)
def test_ragged_call_equals_the_referee(ctx, scale, penalty):
    q_ref, path_ref, value_ref = sc.reference("random", scale, penalty)
    path, q, value = host_call(ctx, sc.random_scores(), sc.WO, scale, penalty)
    assert np.array_equal(q, q_ref)
    assert np.array_equal(value, value_ref)
    assert np.array_equal(path, path_ref)
    if penalty == 1 << 40:     # a constant path: the sign of the sum, a tie falling
        for u in range(len(sc.ROWS)):
            seg = slice(int(sc.WO[u]), int(sc.WO[u + 1]))
            assert (path[seg] == (1 if int(q_ref[seg].astype(np.int64).sum()) > 0 else 0)).all()


@pytest.mark.parametrize("penalty", [0, 1, 3 * 65536, 1 << 40])
def test_adversarial_streams_equal_the_referee(ctx, penalty):
    scores, wo, names = sc.adversarial()
    q_ref, path_ref, value_ref = sc.reference("adversarial", 65536.0, penalty)
    path, q, value = host_call(ctx, scores, wo, 65536.0, penalty)
    assert np.array_equal(q, q_ref)
    assert (q[:int(wo[1])] == 0).all() and q[int(wo[3])] == 0     # 0.5 / 0.5 and the NaN rows
    for u, name in enumerate(names):
        seg = slice(int(wo[u]), int(wo[u + 1]))
        assert np.array_equal(path[seg], path_ref[seg]), name
        assert value[u] == value_ref[u], name
    if penalty == 0:           # q = 0 takes the state of the row after it; the last row is falling
        assert (path[:int(wo[1])] == 0).all()


def test_alone_and_in_a_batch_twice_and_in_both_memory_spaces(ctx):
    scale, penalty = 65536.0, 3 * 65536
    scores = sc.random_scores()
    first = host_call(ctx, scores, sc.WO, scale, penalty)
    again = host_call(ctx, scores, sc.WO, scale, penalty)
    dev = device_call(ctx, scores, sc.WO, scale, penalty)
    for a, b, c in zip(first, again, dev):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    for u in (8, 9):
        lo, hi = int(sc.WO[u]), int(sc.WO[u + 1])
        alone = host_call(ctx, scores[lo:hi], np.array([0, hi - lo], np.int64), scale, penalty)
        assert alone[0].tobytes() == first[0][lo:hi].tobytes() and alone[1].tobytes() == first[1][lo:hi].tobytes()
        assert alone[2][0] == first[2][u]


def test_optional_outputs_and_empty_batches(ctx):
    scores = sc.random_scores()
    wo = sc.WO[:8]
    n = int(wo[-1])
    _, _, value_ref = sc.reference("random", 65536.0, 1)
    path = np.zeros(n, np.uint8)
    ctx.check(ctx.lib.f2_decision_path(ctx.handle, scores.ctypes.data, wo.ctypes.data, len(wo) - 1, 65536.0, 1, path.ctypes.data, None,
                                       None, H))
    assert np.array_equal(path, sc.reference("random", 65536.0, 1)[1][:n])
    value = np.full(3, 5, np.int64)
    ctx.decision_path(None, np.zeros(4, np.int64), 1.0, 0, None, H, value=value)
    assert (value == 0).all()
    assert len(ctx.decision_path(None, np.zeros(1, np.int64), 1.0, 0, None, D)) == 0


def test_argument_errors_leave_the_outputs_alone(ctx):
    scores = sc.random_scores()[:100]
    wo = np.array([0, 40, 100], np.int64)
    path, q, value = np.full(100, 7, np.uint8), np.full(100, -77, np.int32), np.full(2, 5, np.int64)

    def call(scores=scores, wo=wo, U=2, scale=65536.0, penalty=1, path=path, mem=H):
        return ctx.lib.f2_decision_path(ctx.handle, None if scores is None else scores.ctypes.data, None if wo is None else wo.ctypes.data,
                                        U, scale, penalty, None if path is None else path.ctypes.data, q.ctypes.data, value.ctypes.data,
                                        mem)

    inv, uns = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    assert ctx.lib.f2_decision_path(None, scores.ctypes.data, wo.ctypes.data, 2, 1.0, 0, path.ctypes.data, None, None, H) == inv
    assert call(scores=None) == inv and call(path=None) == inv and call(wo=None) == inv and call(U=-1) == inv
    assert call(wo=np.array([1, 40, 100], np.int64)) == inv and call(wo=np.array([0, 50, 40], np.int64)) == inv
    assert call(scale=0.0) == inv and call(scale=-1.0) == inv and call(scale=float("nan")) == inv and call(scale=float("inf")) == inv
    assert call(penalty=-1) == inv and call(mem=2) == inv and call(mem=7) == inv
    assert call(scale=float(2 ** 20) * 1.0000001) == uns and call(penalty=(1 << 40) + 1) == uns
    big = np.array([0, 1 << 31], np.int64)
    assert call(wo=big, U=1) == uns
    assert (path == 7).all() and (q == -77).all() and (value == 5).all()
    assert call(scale=float(2 ** 20), penalty=1 << 40) == _lib.F2_OK      # the limits themselves pass
    assert (path <= 1).all()
