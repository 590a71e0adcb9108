"""f2_interval_tally: decisions per labelled interval against the referee (tests/segments_referee.py), exact - empty and touching
intervals, an interval wholly before the origin, intervals past the last row, hops 1, 7 and 160, fewer interval sets than
utterances, optional path and emissions, host and device memory between guard bands, argument errors."""
import numpy as np
import pytest

import segments_cases as sc
import segments_referee as ref
from devmem import Arena
from f2cnn_amd import _lib

pytestmark = pytest.mark.gpu
H, D = _lib.MEM_HOST, _lib.MEM_DEVICE
ORIGIN = 800
# three utterances per set pass: U = 12 utterances against R = 4 sets (the last utterance is the one that crosses the scan's chunk)
ROWS = sc.ROWS + (300,)
WO = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int64)
N = int(WO[-1])


def interval_sets(hop):
    """R = 4 sets in samples: touching intervals that tile a span, empty ones, one wholly before the origin, ones past every row,
    a set without intervals"""
    far = ORIGIN + hop * (max(ROWS) + 5)
    a = [[0, ORIGIN], [ORIGIN, ORIGIN], [ORIGIN, ORIGIN + 1], [ORIGIN + 1, ORIGIN + 64 * hop], [ORIGIN + 64 * hop, ORIGIN + 65 * hop - 1],
         [ORIGIN + 65 * hop, far], [far, far + 1000]]
    b = [[3, 700], [ORIGIN - 1, ORIGIN + hop * 1024 + 1], [ORIGIN + hop * 1024 + 1, ORIGIN + hop * 2049]]
    # (set 2 serves the long utterance: a long interval, and one that owns its last row alone)
    c = [[ORIGIN + 7, ORIGIN + 7], [ORIGIN + hop * 1000, ORIGIN + hop * 200000], [ORIGIN + hop * 262144, ORIGIN + hop * 262145],
         [far + 5, far + 6]]
    sets = [a, b, c, []]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return offsets, np.array([iv for s in sets for iv in s], np.int64).reshape(-1, 2)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(sc.SEED + 3)
    return (rng.integers(0, 2, N).astype(np.uint8) * 9, rng.integers(0, 2, N).astype(np.uint8),
            rng.integers(-(1 << 24), 1 << 24, N).astype(np.int32))


@pytest.mark.parametrize("hop", [1, 7, 160])
def test_tally_equals_the_referee_in_both_memory_spaces(ctx, rows, hop):
    labels, path, q = rows
    ivo, ivb = interval_sets(hop)
    want = ref.interval_tally(labels, path, q, WO, ivo, ivb, ORIGIN, hop)
    assert len(want) == 3 * int(ivo[-1]) and want[:, 0].max() > 1024 and (want[:, 0] == 0).sum() > 6
    got = ctx.interval_tally(labels, path, q, WO, ivo, ivb, ORIGIN, hop, np.full_like(want, -5), H)
    assert np.array_equal(got, want)
    bare = ctx.interval_tally(labels, None, None, WO, ivo, ivb, ORIGIN, hop, np.full_like(want, -5), H)
    assert np.array_equal(bare[:, :2], want[:, :2]) and (bare[:, 2:] == 0).all()
    with Arena(ctx) as a:
        a.region("labels", np.uint8, N, misalign=1, role="in")
        a.region("path", np.uint8, N, misalign=3, role="in")
        a.region("q", np.int32, N, misalign=1, role="in")
        a.region("tally", np.int64, want.size, misalign=1, role="out")
        for name, arr in (("labels", labels), ("path", path), ("q", q)):
            a.upload(name, arr)
        ctx.interval_tally(a.ptr("labels"), a.ptr("path"), a.ptr("q"), WO, ivo, ivb, ORIGIN, hop, a.ptr("tally"), D)
        ctx.synchronize()
        a.check()
        assert a.download("tally").tobytes() == want.tobytes()


def test_argument_errors(ctx):
    labels = np.zeros(100, np.uint8)
    wo, ivo, ivb = np.array([0, 40, 100], np.int64), np.array([0, 2], np.int64), np.array([[0, 5], [5, 9]], np.int64)
    tally = np.full((4, 4), -5, np.int64)

    def call(labels=labels, wo=wo, U=2, ivo=ivo, ivb=ivb, R=1, origin=0, hop=1, tally=tally, mem=H):
        p = lambda x: None if x is None else x.ctypes.data
        return ctx.lib.f2_interval_tally(ctx.handle, p(labels), None, None, p(wo), U, p(ivo), p(ivb), R, origin, hop, p(tally), mem)

    inv = _lib.F2_ERR_INVALID
    assert call(labels=None) == inv and call(wo=None) == inv and call(ivo=None) == inv and call(ivb=None) == inv and call(tally=None) == inv
    assert call(hop=0) == inv and call(origin=-1) == inv and call(R=0) == inv and call(R=-1) == inv and call(U=-1) == inv and call(mem=2) == inv
    assert call(wo=np.array([0, 40, 100, 100], np.int64), U=3, ivo=np.array([0, 1, 2], np.int64), R=2) == inv     # U % R != 0
    for bad in ([[5, 0], [5, 9]], [[0, 6], [5, 9]], [[-1, 5], [5, 9]]):
        assert call(ivb=np.array(bad, np.int64)) == inv
    assert call(origin=(1 << 63) - 10, hop=1 << 30, wo=np.array([0, 40, 1 << 30], np.int64)) == _lib.F2_ERR_UNSUPPORTED
    assert (tally == -5).all()
    assert call() == _lib.F2_OK and tally[:, 0].tolist() == [5, 4, 5, 4]
