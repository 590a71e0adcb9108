"""f2_decision_runs: maximal runs of equal decisions against the referee (tests/segments_referee.py), exact - random labels at
every row count around a wave, a tile and the scan's chunk, constant and alternating streams, with and without emissions, the
three capacity cases, host and device memory between guard bands, argument errors."""
import numpy as np
import pytest

import segments_cases as sc
import segments_referee as ref
from devmem import Arena
from f2cnn_amd import _lib

pytestmark = pytest.mark.gpu
H, D = _lib.MEM_HOST, _lib.MEM_DEVICE
N = int(sc.WO[-1])


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def streams():
    rng = np.random.default_rng(sc.SEED + 2)
    q = rng.integers(-(1 << 24), 1 << 24, N).astype(np.int32)
    sticky = (np.cumsum(rng.random(N) < 0.01) % 2).astype(np.uint8) * 3     # long runs; nonzero = rising, whatever the value
    return {"random": (rng.integers(0, 2, N).astype(np.uint8), q), "sticky": (sticky, q), "falling": (np.zeros(N, np.uint8), q),
            "rising": (np.full(N, 255, np.uint8), q), "alternating": ((np.arange(N) % 2).astype(np.uint8), q),
            "no emissions": (sticky, None)}


STREAMS = streams()
_ref = {}


def referee(name):
    if name not in _ref:
        _ref[name] = ref.decision_runs(*STREAMS[name], sc.WO)
    return _ref[name]


@pytest.mark.parametrize("name", list(STREAMS))
def test_runs_equal_the_referee_in_both_memory_spaces(ctx, name):
    labels, q = STREAMS[name]
    ro_ref, runs_ref = referee(name)
    if name == "alternating":
        assert len(runs_ref) == N
    if name in ("falling", "rising"):
        assert len(runs_ref) == sum(1 for n in sc.ROWS if n)
    runs = np.full((N, 4), -5, np.int64)
    ro = ctx.decision_runs(labels, q, sc.WO, runs, N, H)
    assert np.array_equal(ro, ro_ref)
    assert np.array_equal(runs[:len(runs_ref)], runs_ref) and (runs[len(runs_ref):] == -5).all()
    with Arena(ctx) as a:
        a.region("labels", np.uint8, N, misalign=1, role="in")
        a.region("q", np.int32, N, misalign=3, role="in")
        a.region("runs", np.int64, 4 * len(runs_ref), misalign=1, role="out")
        a.upload("labels", labels)
        a.upload("q", q if q is not None else np.zeros(N, np.int32))
        ro_d = ctx.decision_runs(a.ptr("labels"), None if q is None else a.ptr("q"), sc.WO, a.ptr("runs"), len(runs_ref), D)
        ctx.synchronize()
        a.check()
        assert a.download("runs").tobytes() == runs_ref.tobytes() and np.array_equal(ro_d, ro_ref)


def test_capacity_exact_one_short_and_counting_only(ctx):
    labels, q = STREAMS["sticky"]
    ro_ref, runs_ref = referee("sticky")
    R = len(runs_ref)
    exact = np.full((R, 4), -5, np.int64)
    assert np.array_equal(ctx.decision_runs(labels, q, sc.WO, exact, R, H), ro_ref) and np.array_equal(exact, runs_ref)
    assert np.array_equal(ctx.decision_runs(labels, q, sc.WO, None, 0, H), ro_ref)
    short, ro = np.full((R, 4), -5, np.int64), np.full(len(sc.WO), -9, np.int64)
    with pytest.raises(_lib.F2Error) as e:
        ctx.decision_runs(labels, q, sc.WO, short, R - 1, H, run_offsets=ro)
    assert e.value.code == _lib.F2_ERR_UNSUPPORTED
    assert np.array_equal(ro, ro_ref) and (short == -5).all()


def test_argument_errors(ctx):
    labels = np.zeros(100, np.uint8)
    wo = np.array([0, 40, 100], np.int64)
    ro, runs = np.full(3, -9, np.int64), np.full((100, 4), -5, np.int64)

    def call(labels=labels, wo=wo, U=2, ro=ro, cap=100, mem=H):
        return ctx.lib.f2_decision_runs(ctx.handle, None if labels is None else labels.ctypes.data, None, None if wo is None else wo.ctypes.data,
                                        U, None if ro is None else ro.ctypes.data, runs.ctypes.data, cap, mem)

    inv = _lib.F2_ERR_INVALID
    assert call(labels=None) == inv and call(wo=None) == inv and call(ro=None) == inv and call(U=-1) == inv and call(cap=-1) == inv
    assert call(wo=np.array([0, 50, 40], np.int64)) == inv and call(mem=2) == inv
    assert call(wo=np.array([0, 1 << 31], np.int64), U=1) == _lib.F2_ERR_UNSUPPORTED
    assert (ro == -9).all() and (runs == -5).all()
    assert np.array_equal(ctx.decision_runs(None, None, np.zeros(3, np.int64), None, 0, H), [0, 0, 0])
