"""f2_occlude_windows against a NumPy model, bit for bit: n windows expanded to K + 1 occlusion levels, window-major. The windows
are random bit patterns (NaNs of every payload among them) and `fill` is stored with its bits, so every comparison is on uint32.
Both memory spaces, device buffers at odd alignments between poisoned guard bands, and argument errors that must write nothing."""
import ctypes

import numpy as np
import pytest

from devmem import Arena
from f2cnn_amd import _lib

pytestmark = pytest.mark.gpu

# (n, R, C, K): one cell; odd sizes; the window shape of the network, 16-byte path; C no multiple of 4, more than one workgroup; more
# than one level group; a plain copy; a host call of more than 16384 output windows (two chunks)
SHAPES = [(1, 1, 1, 1), (3, 3, 5, 4), (2, 11, 128, 16), (257, 11, 67, 3), (2, 11, 128, 1024), (5, 11, 128, 0), (1100, 3, 5, 16)]
NAN_PAYLOAD = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
FILLS = (np.float32(0), np.float32(0.5), NAN_PAYLOAD)
MISALIGN = ((1, 1), (3, 3), (0, 3))     # of x and out, in elements


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def special_patches(R, C):
    """single cells at the four corners, a full row, a full column, the full window, a duplicate, two that overlap"""
    rm, cm = R // 2, C // 2
    return [(0, 1, 0, 1), (0, 1, C - 1, C), (R - 1, R, 0, 1), (R - 1, R, C - 1, C), (rm, rm + 1, 0, C), (0, R, cm, cm + 1), (0, R, 0, C),
            (0, R, cm, cm + 1), (0, rm + 1, 0, cm + 1), (rm, R, cm, C)]


def patches_for(n, R, C, K):
    """K patches: the special ones, starting at a place that differs from shape to shape so that the small K see them all between
    them, then random rectangles"""
    rng = np.random.default_rng(1000 * R + C + K)
    sp = special_patches(R, C)
    first = {4: 0, 3: 4, 1: 6}.get(K, 0)
    out = (sp[first:] + sp[:first])[:K]
    while len(out) < K:
        r0, c0 = int(rng.integers(0, R)), int(rng.integers(0, C))
        out.append((r0, int(rng.integers(r0 + 1, R + 1)), c0, int(rng.integers(c0 + 1, C + 1))))
    return np.array(out, np.int32).reshape(K, 4)


def test_the_patch_sets_cover_the_kinds_the_issue_names():
    seen = set()
    for n, R, C, K in SHAPES:
        P = patches_for(n, R, C, K)
        assert all(0 <= r0 < r1 <= R and 0 <= c0 < c1 <= C for r0, r1, c0, c1 in P)
        rows = [tuple(p) for p in P.tolist()]
        if len(set(rows)) < len(rows):
            seen.add("duplicate")
        for r0, r1, c0, c1 in rows:
            if (r1 - r0, c1 - c0) == (1, 1) and r0 in (0, R - 1) and c0 in (0, C - 1) and R > 1 and C > 1:
                seen.add(("corner", r0 == 0, c0 == 0))
            if r1 - r0 == 1 and c1 - c0 == C and R > 1:
                seen.add("row")
            if r1 - r0 == R and c1 - c0 == 1 and C > 1:
                seen.add("column")
            if (r1 - r0, c1 - c0) == (R, C):
                seen.add("window")
        for a in rows:
            for b in rows:
                if a != b and max(a[0], b[0]) < min(a[1], b[1]) and max(a[2], b[2]) < min(a[3], b[3]):
                    seen.add("overlap")
    assert seen >= {"duplicate", "row", "column", "window", "overlap"} | {("corner", t, l) for t in (True, False) for l in (True, False)}


def windows(n, R, C):
    """random bit patterns: finite values, infinities and NaNs of every payload"""
    return np.random.default_rng(n + 7 * R + 13 * C).integers(0, 2 ** 32, (n, R, C), dtype=np.uint64).astype(np.uint32)


def model(x, P, fill):
    out = np.repeat(x[:, None], len(P) + 1, axis=1)
    bits = np.array([fill], np.float32).view(np.uint32)[0]
    for k, (r0, r1, c0, c1) in enumerate(P):
        out[:, k + 1, r0:r1, c0:c1] = bits
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_host_memory(ctx, shape):
    n, R, C, K = shape
    x, P = windows(n, R, C), patches_for(*shape)
    for fill in FILLS:
        out = np.full((n, K + 1, R, C), 0x7FDEAD01, np.uint32)
        ctx.occlude_windows(x.view(np.float32), n, R, C, P, fill, out.view(np.float32), _lib.MEM_HOST)
        assert np.array_equal(out, model(x, P, fill)), fill


@pytest.mark.parametrize("mis", ((0, 0),) + MISALIGN, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_device_memory_between_guard_bands(ctx, shape, mis):
    n, R, C, K = shape
    x, P = windows(n, R, C), patches_for(*shape)
    for fill in FILLS[1:] if mis != (0, 0) else FILLS:
        with Arena(ctx) as arena:
            arena.region("x", np.float32, x.size, misalign=mis[0], role="in")
            arena.region("out", np.float32, x.size * (K + 1), misalign=mis[1], role="out")
            arena.upload("x", x.view(np.float32))
            ctx.occlude_windows(arena.ptr("x"), n, R, C, P, fill, arena.ptr("out"), _lib.MEM_DEVICE)
            ctx.synchronize()
            arena.check()
            got = arena.download("out").view(np.uint32).reshape(n, K + 1, R, C)
        assert np.array_equal(got, model(x, P, fill)), fill


def test_argument_errors_leave_out_untouched(ctx):
    n0, R0, C0, K0 = 3, 3, 5, 4
    x, P0 = windows(n0, R0, C0).view(np.float32), patches_for(n0, R0, C0, K0)
    out = np.full((n0, K0 + 1, R0, C0), -7.0, np.float32)
    lib = ctx.lib
    A = lambda a: None if a is None else a.ctypes.data

    def call(c=ctx.handle, xx=x, n=n0, R=R0, C=C0, P=P0, K=K0, o=out, mem=_lib.MEM_HOST):
        return lib.f2_occlude_windows(c, A(xx), n, R, C, A(P), K, ctypes.c_float(0.5), A(o), mem)

    def patch(k, col, v):
        Q = P0.copy()
        Q[k, col] = v
        return Q

    invalid = [dict(c=None), dict(xx=None), dict(o=None), dict(P=None), dict(n=-1), dict(R=-1), dict(C=-1), dict(K=-1), dict(mem=3),
               dict(mem=_lib.MEM_HOST_ASYNC), dict(P=patch(1, 0, -1)), dict(P=patch(2, 1, R0 + 1)), dict(P=patch(0, 0, 1)),
               dict(P=patch(3, 2, -1)), dict(P=patch(0, 3, C0 + 1)), dict(P=patch(0, 3, 0))]
    for kw in invalid:
        assert call(**kw) == _lib.F2_ERR_INVALID, kw
    big = np.tile(P0[:1], (1025, 1))
    assert call(P=big, K=1025) == _lib.F2_ERR_UNSUPPORTED
    assert call(n=2 ** 31 // (K0 + 1) + 1) == _lib.F2_ERR_UNSUPPORTED       # (nothing is read: the count alone decides)
    assert (out == -7.0).all()
    assert call(n=0, xx=None, o=None) == _lib.F2_OK
    assert call() == _lib.F2_OK and not (out == -7.0).any()
