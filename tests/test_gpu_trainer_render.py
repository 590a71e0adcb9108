"""f2_input_batch_noisy and the trainer that owns the waves (f2_trainer_set_waves / render / get_windows): the one-call windows
against f2_noise_pick followed by f2_input_batch(F2_WAVE_F64), the trainer's rendered set against f2_input_batch_noisy group by
group, repeatability by seed, training on the rendered set against set_data of the same windows, and the argument errors.
Shapes: tests/noisy_batch.py."""
import numpy as np
import pytest

import noisy_batch as nb
import train_referee as tr
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.trainer import Trainer
from noisy_batch import B, C, K, LEVEL_OF, LENGTHS, R, RADIUS, SEED, SNR, STEP, bits, ptr

pytestmark = pytest.mark.gpu

LR, RHO, EPS, DECAY = 1e-3, 0.9, 1e-7, 0.5


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    with c.options(spectral_min_rows=0):        # the 1 s row takes the spectral route in every call of this module
        yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return nb.coefs()


@pytest.fixture(scope="module")
def corpus():
    """(utterances as int16 arrays, centres per utterance, 0 / 1 signs per utterance)"""
    flat, offsets = nb.waves()
    cs, _ = nb.centers()
    rng = np.random.default_rng(3)
    return [flat[offsets[b]:offsets[b + 1]] for b in range(B)], cs, [rng.integers(0, 2, len(c)).astype(np.uint8) for c in cs]


def noisy_windows(ctx, coefs, flat, dt, offsets, cs, lpf, precision, normalize, snr, level_of, first, seed, mem=_lib.MEM_HOST):
    coff = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    centres = np.concatenate(cs).astype(np.int64)
    n, nbatch = int(coff[-1]), len(offsets) - 1
    out = np.full((n, R, C), np.nan, np.float32)
    if mem == _lib.MEM_HOST:
        ctx.input_batch_noisy(flat, dt, offsets, coefs, nbatch, C, bool(lpf), float(lpf), precision, coff, centres, RADIUS, STEP, normalize,
                              snr, level_of, first, seed, out, mem)
        return out
    d_in, d_out = ctx.malloc(flat.nbytes), ctx.malloc(out.nbytes)
    try:
        ctx.h2d(d_in, flat)
        ctx.h2d(d_out, out)
        ctx.synchronize()
        ctx.input_batch_noisy(d_in, dt, offsets, coefs, nbatch, C, bool(lpf), float(lpf), precision, coff, centres, RADIUS, STEP, normalize,
                              snr, level_of, first, seed, d_out, mem)
        ctx.synchronize()
        ctx.d2h(out, d_out)
        ctx.synchronize()
    finally:
        ctx.free(d_in)
        ctx.free(d_out)
    return out


CASES = [(lpf, norm, _lib.FFT_F32, _lib.MEM_HOST, dt) for lpf in (0, 50) for norm in (0, 1) for dt in (_lib.WAVE_I16, _lib.WAVE_F64)]
CASES += [(50, 1, _lib.FFT_F64, _lib.MEM_HOST, _lib.WAVE_I16), (0, 0, _lib.FFT_F64, _lib.MEM_DEVICE, _lib.WAVE_F64),
          (50, 1, _lib.FFT_F32, _lib.MEM_DEVICE, _lib.WAVE_I16)]


@pytest.mark.parametrize("lpf,normalize,precision,mem,dt", CASES)
def test_one_call_equals_noise_pick_then_input_batch(ctx, coefs, lpf, normalize, precision, mem, dt):
    flat, offsets = nb.waves(dt)
    cs, coff = nb.centers()
    got = noisy_windows(ctx, coefs, flat, dt, offsets, cs, lpf, precision, normalize, SNR, LEVEL_OF, 0, SEED, mem)
    noisy = np.empty(len(flat))
    ctx.noise_pick(flat, dt, offsets, B, SNR, LEVEL_OF, 0, SEED, noisy, _lib.MEM_HOST)
    want = np.full(got.shape, np.nan, np.float32)
    ctx.input_batch(noisy, _lib.WAVE_F64, offsets, coefs, B, C, bool(lpf), float(lpf), precision, coff, np.concatenate(cs), RADIUS, STEP,
                    normalize, want, _lib.MEM_HOST)
    assert len(got) == coff[-1] > B and np.isfinite(got).all()
    assert bits(got).tobytes() == bits(want).tobytes()
    # every utterance clean: still the float64 route, on the converted samples
    clean = noisy_windows(ctx, coefs, flat, dt, offsets, cs, lpf, precision, normalize, (), None, 0, SEED, mem)
    ctx.input_batch(np.asarray(flat, np.float64), _lib.WAVE_F64, offsets, coefs, B, C, bool(lpf), float(lpf), precision, coff,
                    np.concatenate(cs), RADIUS, STEP, normalize, want, _lib.MEM_HOST)
    assert bits(clean).tobytes() == bits(want).tobytes() and not np.array_equal(clean, got)


def new_trainer(ctx, seed=0xABCDEF0123):
    return Trainer(F2CNNModel.glorot(7, R, C, zero_bias=False), lr=LR, rho=RHO, eps=EPS, decay=DECAY, drop=tr.DROP, seed=seed, ctx=ctx)


def rendered(ctx, coefs, corpus, group, snr=SNR, level_of=LEVEL_OF, seed=SEED, lpf=False):
    waves, cs, signs = corpus
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, coefs, RADIUS, STEP, lpf=lpf, cutoff=50.0 if lpf else 0.0, group=group)
    assert (t.ctx.trainer_info(t.handle, "windows"), t.ctx.trainer_info(t.handle, "utterances")) == (sum(len(c) for c in cs), B)
    t.render(snr, level_of, seed)
    x, y = t.windows()
    t.close()
    return x, y


def test_render_is_input_batch_noisy_group_by_group(ctx, coefs, corpus):
    """The contract is per group: group g of a render is f2_input_batch_noisy on those utterances with first_utterance = g group.
    A render in one group (group = 64) is the one-call result by that same contract; that it also equals the group = 2 render is
    NOT part of the contract - an envelope may take another kernel route in another batch composition - so whether they agree is
    printed and not asserted."""
    waves, cs, signs = corpus
    flat, offsets = nb.waves()
    lev = np.array(LEVEL_OF, np.int32)
    for lpf in (False, True):
        x2, y2 = rendered(ctx, coefs, corpus, 2, lpf=lpf)
        assert np.array_equal(y2, np.concatenate(signs))
        row = 0
        for g in range(0, B, 2):
            part = slice(int(offsets[g]), int(offsets[g + 2]))
            want = noisy_windows(ctx, coefs, flat[part], _lib.WAVE_I16, offsets[g:g + 3] - offsets[g], cs[g:g + 2], 50 if lpf else 0,
                                 _lib.FFT_F32, 1, SNR, lev[g:g + 2], g, SEED)
            assert bits(x2[row:row + len(want)]).tobytes() == bits(want).tobytes(), (lpf, g)
            row += len(want)
        assert row == len(x2)
        x64, _ = rendered(ctx, coefs, corpus, 64, lpf=lpf)
        one = noisy_windows(ctx, coefs, flat, _lib.WAVE_I16, offsets, cs, 50 if lpf else 0, _lib.FFT_F32, 1, SNR, lev, 0, SEED)
        assert bits(x64).tobytes() == bits(one).tobytes(), lpf
        print("lpf {}: group 2 and group 64 renders bit-identical: {}, max difference {:.3g}".format(
            lpf, np.array_equal(x2, x64), float(np.abs(x2 - x64).max())))


def test_render_again_same_bytes_other_seed_other_noise(ctx, coefs, corpus):
    waves, cs, signs = corpus
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, coefs, RADIUS, STEP, group=2)
    t.render(SNR, LEVEL_OF, SEED)
    a, _ = t.windows()
    t.render(SNR, LEVEL_OF, SEED + 1)
    c, _ = t.windows()
    t.render(SNR, LEVEL_OF, SEED)
    b, _ = t.windows()
    t.render()
    clean, _ = t.windows()
    part, part_y = t.windows(first=3, count=4)
    t.close()
    assert bits(a).tobytes() == bits(b).tobytes()
    assert bits(part).tobytes() == bits(clean[3:7]).tobytes() and np.array_equal(part_y, np.concatenate(signs)[3:7])
    coff = np.concatenate([[0], np.cumsum([len(x) for x in cs])])
    for u, l in enumerate(LEVEL_OF):
        s = slice(int(coff[u]), int(coff[u + 1]))
        if s.stop > s.start:
            assert np.array_equal(a[s], c[s]) == (l == K), u
            assert np.array_equal(a[s], clean[s]) == (l == K), u


def test_training_on_the_rendered_set_is_training_on_those_windows(ctx, coefs):
    """70 windows in steps of 32, 32 and 6: set_waves + render + steps against set_data(those windows, signs) + steps"""
    lengths = (1500, 3001, 4096, 2000, 1777)
    flat, offsets = nb.waves(lengths=lengths, seed=70)
    cs, coff = nb.centers(lengths, per=(14,))
    assert coff[-1] == 70
    rng = np.random.default_rng(8)
    signs = [rng.integers(0, 2, len(c)).astype(np.uint8) for c in cs]
    waves = [flat[offsets[b]:offsets[b + 1]] for b in range(len(lengths))]
    order = rng.permutation(70).astype(np.int64)
    a = new_trainer(ctx)
    a.set_waves(waves, cs, signs, coefs, RADIUS, STEP, group=2)
    a.render(SNR, [0, 3, 1, 2, 3], SEED)
    x, y = a.windows()
    tally_a = a.steps(order, 32)
    b = new_trainer(ctx)
    b.set_data(x, y)
    assert b.ctx.trainer_info(b.handle, "utterances") == 0
    tally_b = b.steps(order, 32)
    assert a.iterations == b.iterations == 3 and tally_a == tally_b
    for what in ("weights", "accumulators", "gradient"):
        wa, wb = a._get(what), b._get(what)
        for k in tr.TENSORS:
            assert wa[k].tobytes() == wb[k].tobytes(), (what, k)
    # set_data after set_waves: the waves are gone; set_waves after set_data: the windows come from the waves again
    a.set_data(x[:5], y[:5])
    assert a.ctx.trainer_info(a.handle, "windows") == 5 and a.ctx.trainer_info(a.handle, "utterances") == 0
    with pytest.raises(_lib.F2Error) as ei:
        a.render()
    assert ei.value.code == _lib.F2_ERR_INVALID and "no waves" in str(ei.value)
    b.set_waves(waves, cs, signs, coefs, RADIUS, STEP, group=2)
    b.render(SNR, [0, 3, 1, 2, 3], SEED)
    x2, y2 = b.windows()
    assert bits(x2).tobytes() == bits(x).tobytes() and np.array_equal(y2, y)
    a.close()
    b.close()


def test_empty_corpora(ctx, coefs):
    t = new_trainer(ctx)
    with pytest.raises(_lib.F2Error, match="no waves"):
        t.render()
    t.set_waves([], [], [], coefs, RADIUS, STEP)
    t.render(SNR, None, 1)
    assert t.windows()[0].shape == (0, R, C)
    short = [np.zeros(0, np.int16), np.ones(2 * nb.REACH, np.int16)]            # empty, and one sample short of a window
    t.set_waves(short, [np.zeros(0, np.int64)] * 2, [np.zeros(0, np.uint8)] * 2, coefs, RADIUS, STEP)
    t.render(SNR, [0, 1], 1)
    assert t.windows()[0].shape == (0, R, C) and t.ctx.trainer_info(t.handle, "utterances") == 2
    t.close()


def test_errors_change_nothing(ctx, coefs, corpus):
    waves, cs, signs = corpus
    flat, offsets = nb.waves()
    coff = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    centres, sg = np.concatenate(cs), np.concatenate(signs)
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, coefs, RADIUS, STEP, group=2)
    t.render(SNR, LEVEL_OF, SEED)
    before, _ = t.windows()

    def set_waves(wave=flat, dt=_lib.WAVE_I16, off=offsets, channels=C, cen=centres, s=sg, radius=RADIUS, group=2, lpf=0, cutoff=0.0):
        return ctx.lib.f2_trainer_set_waves(ctx.handle, t.handle, ptr(wave), dt, ptr(off), ptr(coefs), B, channels, lpf, cutoff, _lib.FFT_F32,
                                            ptr(coff), ptr(cen), ptr(s), radius, STEP, group)

    outside, late, bad_sign = centres.copy(), centres.copy(), sg.copy()
    outside[coff[1]] = nb.REACH - 1
    late[coff[4] - 1] = LENGTHS[3] - nb.REACH
    bad_sign[7] = 2
    cases = [(dict(channels=C + 1), "windows"), (dict(radius=RADIUS + 1), "windows"), (dict(group=0), "group"), (dict(s=bad_sign), "signs[7]"),
             (dict(cen=outside), "utterance 1"), (dict(cen=late), "utterance 3"), (dict(dt=9), "wave_dtype"), (dict(lpf=1, cutoff=9000.0), "cutoff"),
             (dict(wave=None), "null"), (dict(s=None), "signs")]
    for kw, word in cases:
        rc = set_waves(**kw)
        msg = ctx.lib.f2_last_error(ctx.handle).decode()
        assert rc == _lib.F2_ERR_INVALID and word in msg, (kw.keys(), rc, msg)
        if "cen" in kw:
            assert str(LENGTHS[1 if kw["cen"] is outside else 3]) in msg and "centre" in msg
        assert t.ctx.trainer_info(t.handle, "windows") == len(before) and bits(t.windows()[0]).tobytes() == bits(before).tobytes(), kw.keys()

    bad_level = np.array(LEVEL_OF, np.int32)
    bad_level[5] = K + 1
    nan_snr = np.array(SNR)
    nan_snr[2] = np.nan
    for snr, k, lev, code, word in ((np.array(SNR), K, bad_level, _lib.F2_ERR_INVALID, "utterance 5"),
                                    (nan_snr, K, np.array(LEVEL_OF, np.int32), _lib.F2_ERR_INVALID, "snr_db[2]"),
                                    (None, K, np.array(LEVEL_OF, np.int32), _lib.F2_ERR_INVALID, "snr_db is NULL"),
                                    (np.array(SNR), -1, None, _lib.F2_ERR_INVALID, "K=-1")):
        rc = ctx.lib.f2_trainer_render(ctx.handle, t.handle, ptr(snr), k, ptr(lev), SEED)
        msg = ctx.lib.f2_last_error(ctx.handle).decode()
        assert rc == code and word in msg, (rc, msg)
        assert bits(t.windows()[0]).tobytes() == bits(before).tobytes()
    x = np.empty((1, R, C), np.float32)
    for first, count in ((-1, 1), (0, len(before) + 1), (len(before), 1), (0, -1)):
        assert ctx.lib.f2_trainer_get_windows(ctx.handle, t.handle, first, count, ptr(x), None) == _lib.F2_ERR_INVALID
    t.close()


def test_nonpositive_comes_back_from_render(ctx, coefs):
    """Silence: an all-zero envelope, which the normaliser refuses as it does in f2_input_batch"""
    wave = np.zeros(3000, np.int16)
    t = new_trainer(ctx)
    t.set_waves([wave], [np.array([2500], np.int64)], [np.array([1], np.uint8)], coefs, RADIUS, STEP)
    with pytest.raises(_lib.F2Error) as ei:
        t.render()
    assert ei.value.code == _lib.F2_ERR_NONPOSITIVE
    t.close()
