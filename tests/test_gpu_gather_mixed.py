"""f2_gather_windows_mixed: the ragged window gather with a mixing matrix per utterance.

1. on raw bytes against the two calls it fuses: f2_channel_mix_levels of the same envelopes, then f2_gather_windows per utterance on
   the block of the utterance's level (the pattern of tests/test_gpu_input_from_wav.py's two_step);
2. against NumPy on data whose sums are exact in float64, and within one float32 ulp of NumPy's normaliser;
3. without levels it is the plain gather;
4. the contract of include/f2cnn_hip.h: what a window does not depend on, a row of zeros, and the errors, which write nothing.
"""
import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib, smear

pytestmark = pytest.mark.gpu

LENGTHS = (400, 1500, 640, 977, 1203)          # utterance 2 has no centres
PER = (3, 5, 0, 4, 2)
B = len(LENGTHS)
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
K = 4
MIX_OF = (1, 4, 2, 0, 3)                        # every level and the sharp one (K)
CHANNELS = (1, 5, 33, 128)
SHAPES = ((0, 1), (0, 16), (5, 1), (5, 16))     # (radius, step)
FILL = 0x5A
INV, UNS, NONPOS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED, _lib.F2_ERR_NONPOSITIVE


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def envelopes(C, lengths=LENGTHS, seed=3):
    """positive random ragged (C, n_b) blocks, flat"""
    rng = np.random.default_rng(seed + C)
    return np.concatenate([(rng.random((C, n)) * 40 + 1e-3).reshape(-1) for n in lengths])


def ragged_rows(C, seed=9):
    """a matrix whose rows have zeros inside their supports and supports of unequal width, the ends of a support positive"""
    rng = np.random.default_rng(seed + C)
    W = np.zeros((C, C))
    for c in range(C):
        width = int(rng.integers(1, C + 1))
        lo = int(rng.integers(0, C - width + 1))
        row = rng.random(width) + 0.05
        row[rng.random(width) < 0.4] = 0.0
        row[0], row[-1] = 0.3, 0.7
        W[c, lo:lo + width] = row
    return W


def matrices(C):
    freqs = orc.centre_freqs(16000, C, 100)
    return np.stack([smear.SmearMatrix(freqs, 1.0), smear.BandMatrix(C, min(3, C)), np.eye(C), ragged_rows(C)])


def centres(radius, step, lengths=LENGTHS, per=PER, seed=11):
    """(centres per utterance, center_offsets): the first and the last legal centre of every utterance that has centres"""
    rng = np.random.default_rng(seed)
    reach, cs = radius * step, []
    for n, k in zip(lengths, per):
        c = rng.integers(reach, n - reach, size=k).astype(np.int64)
        if k:
            c[0], c[-1] = reach, n - 1 - reach
        cs.append(c)
    return cs, np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)


def plain_gather(ctx, env, C, offsets, cs, radius, step, normalize):
    """f2_gather_windows per utterance: the plain gather of a ragged batch"""
    out = []
    for b, c in enumerate(cs):
        if len(c):
            e = np.ascontiguousarray(env[C * offsets[b]:C * offsets[b + 1]].reshape(C, -1))
            w = np.empty((len(c), 2 * radius + 1, C), np.float32)
            ctx.gather_windows(e, C, e.shape[1], np.ascontiguousarray(c), len(c), radius, step, normalize, w, _lib.MEM_HOST)
            out.append(w)
    return np.concatenate(out) if out else np.zeros((0, 2 * radius + 1, C), np.float32)


def mixed(ctx, env, C, offsets, cs, coff, radius, step, normalize, mixes, mix_of, mem=_lib.MEM_HOST):
    out = np.full((int(coff[-1]), 2 * radius + 1, C), np.nan, np.float32)
    flat = np.concatenate(cs) if len(cs) else np.zeros(0, np.int64)
    args = (offsets, len(offsets) - 1, C, coff, flat, radius, step, normalize, mixes, mix_of)
    if mem == _lib.MEM_HOST:
        ctx.gather_windows_mixed(env, *args, out, mem)
        return out
    d_in, d_out = ctx.malloc(env.nbytes), ctx.malloc(max(out.nbytes, 8))
    try:
        ctx.h2d(d_in, env)
        ctx.h2d(d_out, out)
        ctx.synchronize()
        ctx.gather_windows_mixed(d_in, *args, d_out, mem)
        ctx.synchronize()
        ctx.d2h(out, d_out)
        ctx.synchronize()
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    return out


_levels = {}


def sweep_levels(ctx, C):
    """(env, matrices, the K + 1 levels of f2_channel_mix_levels): computed once per C, never written to"""
    if C not in _levels:
        env, mix = envelopes(C), matrices(C)
        lev = np.empty((K + 1) * C * int(OFFSETS[-1]))
        ctx.channel_mix_levels(env, OFFSETS, B, C, mix, lev, _lib.MEM_HOST)
        for a in (env, mix, lev):
            a.setflags(write=False)
        _levels[C] = env, mix, lev.reshape(K + 1, -1)
    return _levels[C]


@pytest.mark.parametrize("mem", (_lib.MEM_HOST, _lib.MEM_DEVICE))
@pytest.mark.parametrize("C", CHANNELS)
def test_bit_identical_to_the_sweep_then_the_plain_gather(ctx, C, mem):
    env, mix, lev = sweep_levels(ctx, C)
    for radius, step in SHAPES:
        cs, coff = centres(radius, step)
        for normalize in (0, 1):
            got = mixed(ctx, env, C, OFFSETS, cs, coff, radius, step, normalize, mix, MIX_OF, mem)
            want = []
            for b in range(B):      # utterance b alone, from the block of its level
                only = [c if u == b else c[:0] for u, c in enumerate(cs)]
                want.append(plain_gather(ctx, lev[MIX_OF[b]], C, OFFSETS, only, radius, step, normalize))
            want = np.concatenate(want)
            assert len(got) == sum(PER) and np.isfinite(got).all()
            assert bits(got).tobytes() == bits(want).tobytes(), (radius, step, normalize)
            if C > 1:               # the mixing is there: the sharp gather gives other windows
                assert not np.array_equal(got, plain_gather(ctx, env, C, OFFSETS, cs, radius, step, normalize))


@pytest.mark.parametrize("C", CHANNELS)
def test_against_numpy(ctx, C):
    """integer envelopes in 1 .. 1000 and integer weights in 0 .. 3: every partial sum is an integer below 2^53, exact in float64 in
    any order, so normalize = 0 is (W @ env)[:, taps] exactly. The normaliser within one float32 ulp of NumPy's in float64."""
    rng = np.random.default_rng(77 + C)
    env = np.concatenate([rng.integers(1, 1001, (C, n)).astype(np.float64).reshape(-1) for n in LENGTHS])
    mix = rng.integers(0, 4, (K, C, C)).astype(np.float64)
    mix[:, np.arange(C), np.arange(C)] += 1.0                   # no row of zeros: the mixed values stay positive
    radius, step = 5, 16
    cs, coff = centres(radius, step)
    raw = mixed(ctx, env, C, OFFSETS, cs, coff, radius, step, 0, mix, MIX_OF)
    norm = mixed(ctx, env, C, OFFSETS, cs, coff, radius, step, 1, mix, MIX_OF)
    for b in range(B):
        e = env[C * OFFSETS[b]:C * OFFSETS[b + 1]].reshape(C, -1)
        v = e if MIX_OF[b] == K else mix[MIX_OF[b]] @ e
        for j, centre in enumerate(cs[b]):
            taps = centre + step * (np.arange(2 * radius + 1) - radius)
            w = v[:, taps].T                                     # (R, C)
            assert np.array_equal(raw[coff[b] + j], w.astype(np.float32)), (b, j)
            lw = np.log(w)
            ref = ((lw - lw.min()) / (lw.max() - lw.min())).astype(np.float32) if w.max() > w.min() else np.zeros_like(w, np.float32)
            got = norm[coff[b] + j]
            assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.maximum(np.abs(ref), np.abs(got)))).all(), (b, j)


@pytest.mark.parametrize("mem", (_lib.MEM_HOST, _lib.MEM_DEVICE))
@pytest.mark.parametrize("C", (5, 128))
def test_without_levels_it_is_the_plain_gather(ctx, C, mem):
    env, mix, _ = sweep_levels(ctx, C)
    for radius, step in ((0, 1), (5, 16)):
        cs, coff = centres(radius, step)
        for normalize in (0, 1):
            want = plain_gather(ctx, env, C, OFFSETS, cs, radius, step, normalize)
            for mixes, mix_of in ((mix, None), (None, None), (None, (0,) * B), (mix, (K,) * B), (mix[:1], (1,) * B)):
                got = mixed(ctx, env, C, OFFSETS, cs, coff, radius, step, normalize, mixes, mix_of, mem)
                assert bits(got).tobytes() == bits(want).tobytes(), (radius, step, normalize, mix_of)


@pytest.mark.parametrize("C", (33, 128))
def test_a_window_depends_on_its_column_and_its_row_alone(ctx, C):
    env, mix, _ = sweep_levels(ctx, C)
    radius, step = 5, 16
    cs, coff = centres(radius, step)
    ref = mixed(ctx, env, C, OFFSETS, cs, coff, radius, step, 1, mix, MIX_OF)
    blocks = [env[C * OFFSETS[b]:C * OFFSETS[b + 1]] for b in range(B)]

    def of(order, mix_of, mixes=mix):
        """the batch of utterances `order`, each at mix_of[its place]; returns the windows per utterance"""
        off = np.concatenate([[0], np.cumsum([LENGTHS[b] for b in order])]).astype(np.int64)
        sub = [cs[b] for b in order]
        co = np.concatenate([[0], np.cumsum([len(c) for c in sub])]).astype(np.int64)
        out = mixed(ctx, np.concatenate([blocks[b] for b in order]), C, off, sub, co, radius, step, 1, mixes, mix_of)
        return {b: out[co[i]:co[i + 1]] for i, b in enumerate(order)}

    want = {b: ref[coff[b]:coff[b + 1]] for b in range(B)}
    # B and the place in the batch
    for order in ((3,), (4, 3, 1), (1, 0, 3, 4, 2)):
        got = of(order, [MIX_OF[b] for b in order])
        for b in order:
            assert bits(got[b]).tobytes() == bits(want[b]).tobytes(), (order, b)
    # the levels of the other utterances
    got = of(range(B), [MIX_OF[b] if b == 3 else (MIX_OF[b] + 1) % (K + 1) for b in range(B)])
    assert bits(got[3]).tobytes() == bits(want[3]).tobytes()
    assert not np.array_equal(got[0], want[0])
    # K: unused matrices appended (the sharp utterance is then level K + 2)
    more = np.concatenate([mix, mix[::-1][:2]])
    got = of(range(B), [K + 2 if l == K else l for l in MIX_OF], more)
    for b in range(B):
        assert bits(got[b]).tobytes() == bits(want[b]).tobytes(), b


def test_a_row_of_zeros_is_nonpositive(ctx):
    C = 33
    env, mix, _ = sweep_levels(ctx, C)
    radius, step = 5, 16
    cs, coff = centres(radius, step)
    zero_row = mix.copy()
    zero_row[3, 7, :] = 0.0
    mix_of = (1, 4, 2, 3, 0)                                  # utterance 3 alone uses the matrix with the row of zeros
    out = np.full((int(coff[-1]), 2 * radius + 1, C), np.nan, np.float32)
    with pytest.raises(_lib.F2Error) as e:
        ctx.gather_windows_mixed(env, OFFSETS, B, C, coff, np.concatenate(cs), radius, step, True, zero_row, mix_of, out, _lib.MEM_HOST)
    assert e.value.code == NONPOS
    good = mixed(ctx, env, C, OFFSETS, cs, coff, radius, step, 1, mix, mix_of)
    assert (out[coff[3]:coff[4]] == 0).all()                  # zeros, as the plain gather gives for a window with a value <= 0
    keep = np.r_[0:coff[3], coff[4]:coff[-1]]
    assert bits(out[keep]).tobytes() == bits(good[keep]).tobytes()
    # without normalisation the zeros are values like any other
    raw = mixed(ctx, env, C, OFFSETS, cs, coff, radius, step, 0, zero_row, mix_of)
    assert (raw[coff[3]:coff[4], :, 7] == 0).all() and (raw[coff[3]:coff[4], :, 6] > 0).all()


def test_errors_write_nothing(ctx):
    C, radius, step = 5, 2, 3
    env, mix = envelopes(C), matrices(C)
    cs, coff = centres(radius, step)
    cen = np.concatenate(cs)
    out = np.empty((int(coff[-1]), 2 * radius + 1, C), np.float32)
    out.view(np.uint8)[...] = FILL
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731

    def call(env=env, offsets=OFFSETS, B=B, C=C, coff=coff, cen=cen, radius=radius, step=step, mix=mix, K=K,
             mix_of=np.array(MIX_OF, np.int32), out=out, mem=_lib.MEM_HOST):
        return ctx.lib.f2_gather_windows_mixed(ctx.handle, p(env), p(offsets), B, C, p(coff), p(cen), radius, step, 1, p(mix), K, p(mix_of),
                                               p(out), mem)
    far, early, bad_off, bad_coff, nan_mix, low, high = cen.copy(), cen.copy(), OFFSETS.copy(), coff.copy(), mix.copy(), \
        np.array(MIX_OF, np.int32), np.array(MIX_OF, np.int32)
    far[int(coff[1]) - 1] = LENGTHS[0] - radius * step        # the last window of utterance 0 one sample too far
    early[int(coff[3])] = radius * step - 1
    bad_off[2], bad_coff[0], nan_mix[2, 1, 3], low[1], high[4] = bad_off[1] - 1, 1, np.inf, -1, K + 1
    wide = 513
    cases = [(dict(cen=far), INV, "utterance 0"), (dict(cen=early), INV, "utterance 3"), (dict(offsets=bad_off), INV, "offsets"),
             (dict(coff=bad_coff), INV, "center_offsets"), (dict(B=-1), INV, "bad size"), (dict(C=0), INV, "bad size"),
             (dict(radius=-1), INV, "bad size"), (dict(step=-1), INV, "bad size"), (dict(env=None), INV, "null"),
             (dict(cen=None), INV, "null"), (dict(out=None), INV, "null"), (dict(mem=7), INV, ""),
             (dict(K=-1), INV, "K=-1"), (dict(mix=None), INV, "mixing"), (dict(mix=nan_mix), INV, "[2][1][3]"),
             (dict(mix_of=low), INV, "utterance 1"), (dict(mix_of=high), INV, "utterance 4"),
             (dict(mix=np.resize(mix, (65, C, C)), K=65), UNS, "65 mixing matrices"),
             (dict(C=wide, env=np.ones(wide * int(OFFSETS[-1])), mix=np.ones((1, wide, wide)), K=1, mix_of=np.zeros(B, np.int32),
                   out=np.empty(0, np.float32)), UNS, "513 channels"),
             # 21 x (2 * 512 + 1) float64 values are 172 200 bytes of LDS
             (dict(C=512, env=np.ones(512 * int(OFFSETS[-1])), mix=np.ones((1, 512, 512)), K=1, mix_of=np.zeros(B, np.int32), radius=10,
                   step=1, cen=np.full(len(cen), 100, np.int64), out=np.empty(0, np.float32)), UNS, "LDS")]
    for kw, status, word in cases:
        assert call(**kw) == status, list(kw)
        msg = ctx.lib.f2_last_error(ctx.handle).decode()
        assert word in msg, (list(kw), msg)
        assert (bits(out) == FILL).all(), list(kw)
    assert call() == _lib.F2_OK and np.isfinite(out).all()
    # nothing to do is no error, whatever the pointers
    assert call(B=0, offsets=None, coff=None, env=None, cen=None, out=None) == _lib.F2_OK
    assert call(coff=np.zeros(B + 1, np.int64), env=None, cen=None, out=None) == _lib.F2_OK
    assert call(K=0, mix=None) == _lib.F2_OK and call(mix_of=None, mix=None) == _lib.F2_OK
