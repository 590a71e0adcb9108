"""f2_channel_mix_levels: linear maps across the channels of envelopes in memory, at K mixing matrices and as a copy in one pass.
Small ragged batches whose lengths lie around the kernel's time tile (rows start at odd 8-byte offsets), channel counts around
its channel tile, matrices whose supports differ between the rows of one tile - held against NumPy's matrix product (the referee
is written here), on raw bits where every order of the sum is exact, inside the bound between two differently ordered sums on
float data, and on raw bits against themselves (alone / in a batch / K = 1 / K = 64 / host and device memory). Through the C ABI
via ctypes.

The bound on float data is not tuned: two sums of the same m products in different orders differ by at most
2 gamma_m sum |w||x|, gamma_m = m u / (1 - m u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1;
tests/test_gpu_reverb_levels.py uses it the same way); m = C, the longest row."""
import numpy as np
import pytest

from f2cnn_amd import _lib, smear

pytestmark = pytest.mark.gpu

TS, TC = _lib.SMEAR_TILE_SAMPLES, _lib.SMEAR_TILE_CHANNELS
LENGTHS = (3, TS + 1, 0, 1, TS - 1, 2, 2 * TS + 1, TS)       # mixed: most rows start at an odd double index
CHANNELS = (1, 2, TC - 1, TC, TC + 1, 128, 130)
FILL = 0x5A
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def words(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint64)


def offsets_of(lengths):
    o = np.zeros(len(lengths) + 1, np.int64)
    o[1:] = np.cumsum(lengths)
    return o


def blocks_of(flat, offsets, C):
    """the (C, n_b) blocks of a ragged buffer"""
    return [flat[C * offsets[b]:C * offsets[b + 1]].reshape(C, -1) for b in range(len(offsets) - 1)]


def raw_levels(ctx, env, offsets, B, nchan, mix, k, levels, mem_space=_lib.MEM_HOST):
    p = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a)
    return ctx.lib.f2_channel_mix_levels(ctx.handle, p(env), p(offsets), B, nchan, p(mix), k, p(levels), mem_space)


def levels_of(ctx, env, offsets, C, mix):
    mix = np.ascontiguousarray(mix, np.float64).reshape(-1, C, C)
    out = np.empty((len(mix) + 1, env.size), np.float64)
    bits(out)[...] = FILL
    rc = raw_levels(ctx, env, offsets, len(offsets) - 1, C, mix, len(mix), out)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return out


def referee(env, offsets, C, W):
    """W @ env per utterance, a zero as +0.0 (the header's liberty)"""
    out = np.empty_like(env)
    for src, dst in zip(blocks_of(env, offsets, C), blocks_of(out, offsets, C)):
        dst[...] = W @ src + 0.0
    return out


def supports(C, rng, integer):
    """name -> (C, C) matrix; the supports (first .. last non-zero weight of a row) differ between the rows of one channel tile"""
    def weights(shape):
        if integer:
            w = rng.integers(1, 9, shape).astype(np.float64)          # in [-8, 8], never 0 where a weight is meant
            return w * rng.choice([-1.0, 1.0], shape)
        w = rng.standard_normal(shape)
        return np.where(w == 0, 1.0, w)
    c = np.arange(C)
    full = weights((C, C))
    corner = np.zeros((C, C))
    corner[0, C - 1], corner[C - 1, 0] = weights(2)
    lo = np.maximum(0, c - c % 5)
    hi = np.minimum(C, c + 1 + (7 * c) % 4)
    band = full * ((c[None, :] >= lo[:, None]) & (c[None, :] < hi[:, None]))
    holes = band.copy()
    inner = (c[None, :] > lo[:, None]) & (c[None, :] < hi[:, None] - 1) & ((c[None, :] + c[:, None]) % 3 == 0)
    holes[inner] = 0.0                                                # zeros inside the support are walked
    holes[c % 7 == 3] = 0.0                                           # rows of zeros store +0.0
    return {"dense": full, "identity": np.eye(C), "from 0": full * (c[None, :] <= c[:, None]), "to C-1": full * (c[None, :] >= c[:, None]),
            "corner": corner, "band": band, "holes and zero rows": holes}


@pytest.mark.parametrize("C", CHANNELS)
def test_integer_data_gives_the_matrix_product_bit_for_bit(ctx, C):
    """envelopes in [-32768, 32768), weights in [-8, 8]: every partial sum stays below 2^26, so any order of the sum is exact"""
    rng = np.random.default_rng(100 + C)
    offsets = offsets_of(LENGTHS)
    env = rng.integers(-32768, 32768, C * int(offsets[-1])).astype(np.float64)
    mats = supports(C, rng, integer=True)
    levels = levels_of(ctx, env, offsets, C, list(mats.values()))
    for l, (name, W) in enumerate(mats.items()):
        assert np.array_equal(words(levels[l]), words(referee(env, offsets, C, W))), (C, name)
    assert np.array_equal(words(levels[len(mats)]), words(env))                    # level K: the copy
    zero_rows = np.flatnonzero(~mats["holes and zero rows"].any(axis=1))
    for blk in blocks_of(levels[list(mats).index("holes and zero rows")], offsets, C):
        assert (words(blk[zero_rows]) == 0).all()                                  # +0.0, not -0.0


@pytest.mark.parametrize("C,bands", [(16, 4), (128, 8), (TC + 1, TC + 1), (130, 65), (2, 1)])
def test_band_matrices_with_power_of_two_groups_are_exact(ctx, C, bands):
    W = smear.BandMatrix(C, bands)
    sizes = {int(round(1 / w)) for w in W[W > 0]}
    assert all(s & (s - 1) == 0 for s in sizes)                                    # 1 / len(group) is a power of two
    rng = np.random.default_rng(C)
    offsets = offsets_of(LENGTHS)
    env = rng.integers(-32768, 32768, C * int(offsets[-1])).astype(np.float64)
    levels = levels_of(ctx, env, offsets, C, [W])
    assert np.array_equal(words(levels[0]), words(referee(env, offsets, C, W)))
    if bands == C:
        assert np.array_equal(words(levels[0]), words(env))


@pytest.mark.parametrize("C", CHANNELS)
def test_float_data_stays_inside_the_bound_of_two_orders(ctx, C):
    rng = np.random.default_rng(200 + C)
    offsets = offsets_of(LENGTHS)
    env = rng.standard_normal(C * int(offsets[-1])) * np.exp(rng.uniform(-6, 6, C * int(offsets[-1])))   # signed, 5 decades
    mats = supports(C, rng, integer=False)
    freqs = np.geomspace(8000.0, 100.0, C)
    mats["smear 1 ERB"] = smear.SmearMatrix(freqs, 1.0)
    mats["smear 4 ERB"] = smear.SmearMatrix(freqs, 4.0)
    levels = levels_of(ctx, env, offsets, C, list(mats.values()))
    gamma = C * U / (1 - C * U)
    worst = 0.0
    for l, (name, W) in enumerate(mats.items()):
        want, scale = referee(env, offsets, C, W), referee(np.abs(env), offsets, C, np.abs(W))
        err, bound = np.abs(levels[l] - want), 2 * gamma * scale
        assert (err <= bound).all(), (C, name, float((err / np.maximum(bound, 1e-300)).max()))
        if (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"C = {C}: largest error as a fraction of 2 gamma_C |W| @ |env|: {worst:.3g}")
    assert np.array_equal(words(levels[len(mats)]), words(env))
    # the identity: a bit copy up to the sign of a zero
    ident = levels[list(mats).index("identity")]
    assert np.array_equal(words(ident), words(env + 0.0))


def test_a_negative_zero_comes_out_positive_and_the_copy_keeps_it(ctx):
    C = 3
    offsets = offsets_of((5, 2))
    env = np.random.default_rng(1).standard_normal(C * 7)
    env[[0, 4, 9, 20]] = -0.0
    levels = levels_of(ctx, env, offsets, C, [np.eye(C)])
    assert np.array_equal(words(levels[1]), words(env)) and np.signbit(levels[1][[0, 4, 9, 20]]).all()
    assert np.array_equal(levels[0], env) and not np.signbit(levels[0][[0, 4, 9, 20]]).any()


# ---- the bits of a sample depend on its envelope column and its matrix row alone ---------------------------------------------------
IND_C = TC + 1


@pytest.fixture(scope="module")
def independence_case(ctx):
    rng = np.random.default_rng(7)
    offsets = offsets_of(LENGTHS)
    env = rng.standard_normal(IND_C * int(offsets[-1])) * 1e3
    mats = supports(IND_C, rng, integer=False)
    three = [mats["band"], mats["dense"], mats["from 0"]]
    full = levels_of(ctx, env, offsets, IND_C, three)
    for a in (env, full):
        a.setflags(write=False)
    return env, offsets, three, full


def test_alone_and_inside_a_batch_and_at_K_1(ctx, independence_case):
    env, offsets, three, full = independence_case
    assert np.array_equal(bits(levels_of(ctx, env, offsets, IND_C, three)), bits(full))          # a second call
    for b in (LENGTHS.index(2 * TS + 1), LENGTHS.index(1), LENGTHS.index(TS + 1)):
        alone = np.ascontiguousarray(blocks_of(env, offsets, IND_C)[b]).reshape(-1)
        o1 = offsets_of((LENGTHS[b],))
        for l, W in enumerate(three):
            one = levels_of(ctx, alone, o1, IND_C, [W])
            assert np.array_equal(words(one[0]), words(blocks_of(full[l], offsets, IND_C)[b])), (b, l)
            assert np.array_equal(words(one[1]), words(alone))


def test_among_64_levels(ctx, independence_case):
    env, offsets, three, full = independence_case
    rng = np.random.default_rng(8)
    many = [rng.standard_normal((IND_C, IND_C)) * (rng.random((IND_C, IND_C)) < 0.3) for _ in range(64)]
    places = (0, 31, 63)
    for at, W in zip(places, three):
        many[at] = W
    levels = levels_of(ctx, env, offsets, IND_C, many)
    for l, at in enumerate(places):
        assert np.array_equal(words(levels[at]), words(full[l])), at
    assert np.array_equal(words(levels[64]), words(env))
    for at in (1, 40):                                                            # and the others are what NumPy says
        want, scale = referee(env, offsets, IND_C, many[at]), referee(np.abs(env), offsets, IND_C, np.abs(many[at]))
        assert (np.abs(levels[at] - want) <= 2 * IND_C * U / (1 - IND_C * U) * scale).all()


def test_device_memory_and_a_callers_device_buffer(ctx, independence_case):
    env, offsets, three, full = independence_case
    mix = np.ascontiguousarray(three)
    d_env, d_lev = ctx.malloc(env.nbytes), ctx.malloc(full.nbytes)
    try:
        ctx.h2d(d_env, env)
        rc = raw_levels(ctx, d_env, offsets, len(LENGTHS), IND_C, mix, 3, d_lev, _lib.MEM_DEVICE)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        ctx.synchronize()
        got = np.empty_like(full)
        ctx.d2h(got, d_lev)
    finally:
        ctx.synchronize()
        ctx.free(d_env)
        ctx.free(d_lev)
    assert np.array_equal(bits(got), bits(full))
    # the Python binding, host memory
    out = np.empty(full.shape)
    ctx.channel_mix_levels(env, offsets, len(LENGTHS), IND_C, three, out, _lib.MEM_HOST)
    assert np.array_equal(bits(out), bits(full))


# ---- empty calls and errors ---------------------------------------------------------------------------------------------------------
def test_empty_batches(ctx):
    out = np.empty(4)
    bits(out)[...] = FILL
    assert raw_levels(ctx, None, np.zeros(1, np.int64), 0, 3, np.eye(3), 1, None) == _lib.F2_OK
    assert raw_levels(ctx, None, np.zeros(3, np.int64), 2, 3, np.eye(3), 1, out) == _lib.F2_OK
    assert (bits(out) == FILL).all()


@pytest.mark.parametrize("case", ["K=0", "K=65", "mix NULL", "weight nan", "weight inf", "weight -inf", "C=0", "C=513", "B<0",
                                  "offsets NULL", "offsets[0]=1", "offsets decreasing", "env NULL", "levels NULL", "mem_space",
                                  "mem_space async"])
def test_bad_arguments_leave_the_output_alone(ctx, case):
    C = 3
    offsets = offsets_of((65, 2, 63))
    env = np.random.default_rng(3).standard_normal(C * int(offsets[-1]))
    mix, k, nchan, nb, mem, want = np.stack([np.eye(C), np.full((C, C), 0.5)]), 2, C, 3, _lib.MEM_HOST, _lib.F2_ERR_INVALID
    out = np.empty((3, env.size))
    bits(out)[...] = FILL
    dst = out
    if case == "K=0":
        k = 0
    elif case == "K=65":
        mix, k, want = np.zeros((65, C, C)), 65, _lib.F2_ERR_UNSUPPORTED
    elif case == "mix NULL":
        mix = None
    elif case.startswith("weight "):
        mix[1, 2, 0] = float(case.split()[1])
    elif case == "C=0":
        nchan = 0
    elif case == "C=513":
        nchan, want = _lib.SMEAR_MAX_CHANNELS + 1, _lib.F2_ERR_UNSUPPORTED       # (refused before a weight is read)
    elif case == "B<0":
        nb = -1
    elif case == "offsets NULL":
        offsets = None
    elif case == "offsets[0]=1":
        offsets = offsets.copy()
        offsets[0] = 1
    elif case == "offsets decreasing":
        offsets = offsets.copy()
        offsets[2] = offsets[1] - 1
    elif case == "env NULL":
        env = None
    elif case == "levels NULL":
        dst = None
    elif case == "mem_space":
        mem = 7
    else:
        mem = _lib.MEM_HOST_ASYNC
    assert raw_levels(ctx, env, offsets, nb, nchan, mix, k, dst, mem) == want, case
    assert (bits(out) == FILL).all(), case
    if case.startswith("weight "):
        assert "[1][2][0]" in ctx.lib.f2_last_error(ctx.handle).decode()          # level, row, column
