"""f2_lowpass_pick with F2_MEM_DEVICE buffers at placements a caller's tensor slice produces, as
tests/test_gpu_cutoff_sweep_placement.py holds f2_lowpass_levels: every buffer inside one arena (tests/devmem.py) between guard
bands of poison, an odd number of elements past a 256-byte boundary. Asserted per placement: the output equals the host-memory call
on raw bits, every guard band and every input is byte for byte as before, no output element keeps its pre-fill; in place, the one
buffer is both.

What the kernel does to caller-supplied pointers: k_lowpass_pick loads and stores 16-byte pairs through f2_d2u, declared aligned(8)
(f2_envelope_core.h), and single float64 values at an odd tail - element alignment, as the header grants. float64 misalignments
1 / 5 / 15 (120 bytes: a pair store there straddles two 128-byte lines)."""
import numpy as np
import pytest

from devmem import Arena
from f2cnn_amd import _lib

pytestmark = pytest.mark.gpu

F64 = np.float64
DEV, HOST = _lib.MEM_DEVICE, _lib.MEM_HOST
C = 3
LENS = [65, 1, 4097, 0, 2, 8193, 63]           # odd lengths: rows start at odd 8-byte offsets; the 4096-sample segment edge
CUTOFFS = (5.0, 50.0, 7900.0)
CUTOFF_OF = (0, 3, 1, 2, 3, 2, 3)              # every level; unfiltered rows between filtered ones
B = len(LENS)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(ctx):
    """the batch and the host-memory call: computed once, only read"""
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    env = np.random.default_rng(9).standard_normal(C * int(off[-1]))
    host = np.empty(env.size)
    ctx.lowpass_pick(env, off, B, C, CUTOFFS, CUTOFF_OF, host, HOST)
    for a in (off, env, host):
        a.setflags(write=False)
    return off, env, host


def same_bits(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("env_mis,out_mis", [(0, 0), (1, 1), (5, 15), (15, 5), (0, 1), (1, 0)])
def test_out_of_place(ctx, case, env_mis, out_mis):
    off, env, host = case
    with Arena(ctx) as a:
        a.region("env", F64, env.size, misalign=env_mis, role="in")
        a.region("filtered", F64, env.size, misalign=out_mis, role="out")
        a.upload("env", env)
        ctx.lowpass_pick(a.ptr("env"), off, B, C, CUTOFFS, CUTOFF_OF, a.ptr("filtered"), DEV)
        ctx.synchronize()
        a.check()
        assert a.unwritten("filtered") == 0
        assert same_bits(a.download("filtered"), host)


@pytest.mark.parametrize("mis", [0, 1, 5, 15])
def test_in_place(ctx, case, mis):
    off, env, host = case
    with Arena(ctx) as a:
        a.region("env", F64, env.size, misalign=mis, role="inout")
        a.region("other", F64, 64, misalign=1, role="in")            # a bystander: nothing but the one buffer changes
        a.upload("env", env)
        a.upload("other", np.arange(64.0))
        ctx.lowpass_pick(a.ptr("env"), off, B, C, CUTOFFS, CUTOFF_OF, a.ptr("env"), DEV)
        ctx.synchronize()
        a.check()
        assert same_bits(a.download("env"), host)


def test_an_unfiltered_batch_in_place_leaves_its_pre_fill(ctx, case):
    """every utterance at level K, in place, on a region that was never uploaded: the poison of the arena is all still there"""
    off, env, _ = case
    with Arena(ctx) as a:
        a.region("env", F64, env.size, misalign=5, role="inout")
        ctx.lowpass_pick(a.ptr("env"), off, B, C, CUTOFFS, (len(CUTOFFS),) * B, a.ptr("env"), DEV)
        ctx.synchronize()
        a.check()
        assert a.unwritten("env") == env.size
