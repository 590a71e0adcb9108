"""f2_eval_noise_sweep: a ragged batch at K noise levels and clean in one device pass. The noise is held against a NumPy
restatement of the header's generator (Philox4x32-10 -> two 53-bit uniforms -> Box-Muller cosine branch), sigma against
NumPy, the evaluation - on raw bits - against f2_eval_batch_strided(F2_WAVE_F64) on the waveforms the call returns, and the
device's tally against counts made from the returned labels. All through the C ABI via ctypes, as tests/test_gpu_eval_strided.py."""
import ctypes
import os

import numpy as np
import pytest

import f2cnn_oracle as orc
import speechlike
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

C, RADIUS, STEP = 128, 5, 160
R = 2 * RADIUS + 1
LENGTHS = (1761, 4000, 1700, 0)          # one window, a few thousand, none (n <= 11 * step), empty
B = len(LENGTHS)
SNR = (10.0, -3.0)
K = len(SNR)
U = (K + 1) * B
SEED = 0x1234_5678_9ABC
FILL = 0x5A

# ---- the generator of include/f2cnn_hip.h (f2_eval_noise_sweep), restated ---------------------------------------------------
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two; -> four uint64 arrays holding the 32-bit output words"""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2        # 32 x 32 -> 64 bit: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def deviates(seed, level, utt, n):
    """z of samples 0 .. n-1 of utterance `utt` at level `level`"""
    i = np.arange(n, dtype=np.uint64)
    w0, w1, w2, w3 = philox4x32_10((i & MASK, i >> np.uint64(32), level, utt), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((w0 >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (w1 >> np.uint64(6)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = ((w2 >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (w3 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def test_restatement_gives_the_published_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = " ".join("{:08x}".format(int(w)) for w in philox4x32_10(counter, key))
        assert got == want, (counter, key)
    z = deviates(SEED, 0, 1, 4000)
    assert np.isfinite(z).all() and np.abs(z).max() < 8.6 and abs(z.mean()) < 0.1 and abs(z.std() - 1) < 0.1


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))


@pytest.fixture(scope="module")
def model():
    return F2CNNModel(orc.glorot_weights(7))


def ragged_waves(lengths, seed=40):
    """as tests/test_gpu_eval_strided.py builds its batch: the 4000-sample utterance is speech-shaped"""
    waves = []
    for i, n in enumerate(lengths):
        waves.append(speechlike.make(seed + i, n, "syllables")[0] if n == 4000 else orc.synth_utterance(seed + i, n))
    offsets = np.zeros(len(lengths) + 1, np.int64)
    offsets[1:] = np.cumsum(lengths)
    return np.concatenate(waves).astype(np.int16), offsets


@pytest.fixture(scope="module")
def batch():
    return ragged_waves(LENGTHS)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def tiled_offsets(offsets, levels):
    total = int(offsets[-1])
    return np.concatenate([[0]] + [l * total + offsets[1:] for l in range(levels)]).astype(np.int64)


def n_windows(hop, levels=K + 1):
    return levels * sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in LENGTHS)


class Out:
    """every output of one call, pre-filled with 0x5A"""

    def __init__(self, total, hop, levels=K + 1):
        self.noisy = filled(levels * total, np.float64)
        self.scores = filled((n_windows(hop, levels), 2), np.float32)
        self.labels = filled(n_windows(hop, levels), np.uint8)
        self.wo = filled(levels * B + 1, np.int64)
        self.sigma = filled(levels * B, np.float64)
        self.stats = filled((levels * B, 2), np.int64)

    def untouched(self):
        return all((bits(a) == FILL).all() for a in (self.noisy, self.scores, self.labels, self.wo, self.sigma, self.stats))


def raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, snr, k, seed, o, lpf=False, want_scores=True, want_labels=True,
              nbatch=B):
    p = lambda a: None if a is None else a.ctypes.data
    return ctx.lib.f2_eval_noise_sweep(ctx.handle, model.handle(ctx), p(wave), dtype, p(offsets), p(coefs), nbatch, C, int(lpf),
                                       50.0 if lpf else 0.0, _lib.FFT_F32, RADIUS, STEP, hop, p(snr), k, seed, p(o.noisy),
                                       p(o.scores) if want_scores else None, p(o.labels) if want_labels else None, p(o.wo),
                                       p(o.sigma), p(o.stats), _lib.MEM_HOST)


def sweep(ctx, model, coefs, wave, dtype, offsets, hop, lpf=False, seed=SEED, **kw):
    o = Out(int(offsets[-1]), hop)
    rc = raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, np.array(SNR), K, seed, o, lpf=lpf, **kw)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return o


@pytest.fixture(scope="module")
def frame_sweep(ctx, model, coefs, batch):
    """the int16 batch at hop 160 without low-pass: shared by the tests that only read it"""
    flat, offsets = batch
    return sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160)


def numpy_sigma(flat, offsets):
    want = np.zeros(U)
    for l, snr in enumerate(SNR):
        for b in range(B):
            w = flat[offsets[b]:offsets[b + 1]]
            if len(w):
                want[l * B + b] = np.sqrt(np.mean(np.square(w.astype(np.float64)))) / 10 ** (snr / 10)
    return want


# ---- 1. sigma ---------------------------------------------------------------------------------------------------------------
def test_sigma_int16_is_numpys_to_one_ulp(batch, frame_sweep):
    flat, offsets = batch
    got, want = frame_sweep.sigma, numpy_sigma(flat, offsets)
    print("sigma", got, "numpy", want)
    assert (np.abs(got - want) <= np.spacing(want)).all()
    assert (got[K * B:] == 0).all() and (bits(got[K * B:]) == 0).all()           # the clean level
    assert all(got[l * B + 3] == 0 for l in range(K + 1))                        # the empty utterance
    assert (got[:K * B].reshape(K, B)[:, :3] > 0).all()


def test_sigma_float64_in_a_fixed_order(ctx, model, coefs, batch):
    flat, offsets = batch
    f64 = flat.astype(np.float64)
    a = sweep(ctx, model, coefs, f64, _lib.WAVE_F64, offsets, 160)
    b = sweep(ctx, model, coefs, f64, _lib.WAVE_F64, offsets, 160)
    want = numpy_sigma(flat, offsets)
    rel = np.abs(a.sigma - want) / np.where(want > 0, want, 1)
    print("max relative difference to numpy", rel.max())
    assert rel.max() <= 1e-14
    assert (a.sigma[want == 0] == 0).all()
    assert np.array_equal(bits(a.sigma), bits(b.sigma))


# ---- 2. noise ---------------------------------------------------------------------------------------------------------------
def test_noise_is_the_headers_generator(batch, frame_sweep):
    flat, offsets = batch
    total = int(offsets[-1])
    noisy, sigma = frame_sweep.noisy.reshape(K + 1, total), frame_sweep.sigma
    assert np.array_equal(noisy[K], flat.astype(np.float64))                     # the clean level, exactly
    worst = 0.0
    for l in range(K):
        for b, n in enumerate(LENGTHS):
            clean = flat[offsets[b]:offsets[b + 1]].astype(np.float64)
            s = sigma[l * B + b]
            want = clean + s * deviates(SEED, l, b, n)
            err = np.abs(noisy[l, offsets[b]:offsets[b + 1]] - want)
            bound = 2.0 ** -52 * np.abs(want) + 1e-13 * s
            if n:
                worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (l, b, float((err / bound).max()))
    print("worst error / bound", worst)


def test_levels_are_different_streams(batch, frame_sweep):
    flat, offsets = batch
    total = int(offsets[-1])
    noisy, sigma = frame_sweep.noisy.reshape(K + 1, total), frame_sweep.sigma
    lo, hi = offsets[1], offsets[2]                                              # the 4000-sample row
    clean = flat[lo:hi].astype(np.float64)
    z = [(noisy[l, lo:hi] - clean) / sigma[l * B + 1] for l in range(K)]         # both levels at sigma = 1
    r = float(np.corrcoef(z[0], z[1])[0, 1])
    print("correlation of levels 0 and 1", r)
    assert abs(r) < 0.1
    assert abs(float(np.corrcoef(deviates(SEED, 0, 1, 4000), deviates(SEED, 1, 1, 4000))[0, 1])) < 0.1


def test_seed_decides_the_noise(ctx, model, coefs, batch, frame_sweep):
    flat, offsets = batch
    again = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160)
    assert np.array_equal(bits(again.noisy), bits(frame_sweep.noisy))
    other = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, seed=SEED + 1)
    total = int(offsets[-1])
    assert not np.array_equal(bits(other.noisy[:K * total]), bits(frame_sweep.noisy[:K * total]))
    assert np.array_equal(bits(other.noisy[K * total:]), bits(frame_sweep.noisy[K * total:]))
    assert np.array_equal(bits(other.sigma), bits(frame_sweep.sigma))


# ---- 3. composition: no tolerance ---------------------------------------------------------------------------------------------
def strided_on(ctx, model, coefs, noisy, offsets, hop, lpf):
    t = tiled_offsets(offsets, K + 1)
    sc, lb = filled((n_windows(hop), 2), np.float32), filled(n_windows(hop), np.uint8)
    wo = ctx.eval_batch_strided(model.handle(ctx), noisy, _lib.WAVE_F64, t, coefs, U, C, lpf, 50.0 if lpf else 0.0, _lib.FFT_F32,
                                RADIUS, STEP, hop, sc, lb, _lib.MEM_HOST)
    return sc, lb, wo


@pytest.mark.parametrize("hop,lpf", [(160, False), (160, True), (7, False), (7, True), (1, True)])
def test_evaluation_is_the_strided_call_on_the_returned_waveforms(ctx, model, coefs, batch, hop, lpf):
    flat, offsets = batch
    o = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, lpf=lpf)
    sc, lb, wo = strided_on(ctx, model, coefs, o.noisy, offsets, hop, lpf)
    assert np.array_equal(o.wo, wo) and o.wo[-1] == n_windows(hop) > 0
    assert np.array_equal(bits(o.scores), bits(sc))
    assert np.array_equal(o.labels, lb) and set(np.unique(o.labels)) <= {0, 1}


def test_device_buffers(ctx, model, coefs, batch, frame_sweep):
    flat, offsets = batch
    hop, total = 160, int(offsets[-1])
    o = Out(total, hop)
    dev = [ctx.malloc(max(a.nbytes, 8)) for a in (flat, o.noisy, o.scores, o.labels)]
    try:
        for p, a in zip(dev, (flat, o.noisy, o.scores, o.labels)):
            ctx.h2d(p, a)
        snr = np.array(SNR)
        rc = ctx.lib.f2_eval_noise_sweep(ctx.handle, model.handle(ctx), dev[0], _lib.WAVE_I16, offsets.ctypes.data, coefs.ctypes.data, B,
                                         C, 0, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, snr.ctypes.data, K, SEED, dev[1], dev[2], dev[3],
                                         o.wo.ctypes.data, o.sigma.ctypes.data, o.stats.ctypes.data, _lib.MEM_DEVICE)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        for p, a in zip(dev[1:], (o.noisy, o.scores, o.labels)):
            ctx.d2h(a, p)
    finally:
        ctx.synchronize()
        for p in dev:
            ctx.free(p)
    for name in ("noisy", "scores", "labels", "wo", "sigma", "stats"):
        assert np.array_equal(bits(getattr(o, name)), bits(getattr(frame_sweep, name))), name
    sc, lb, wo = strided_on(ctx, model, coefs, o.noisy, offsets, hop, False)
    assert np.array_equal(bits(o.scores), bits(sc)) and np.array_equal(o.labels, lb) and np.array_equal(o.wo, wo)


# ---- 4. tally -----------------------------------------------------------------------------------------------------------------
def numpy_stats(labels, wo):
    want = np.zeros((U, 2), np.int64)
    for u in range(U):
        mine = labels[wo[u]:wo[u + 1]]
        clean = labels[wo[K * B + u % B]:wo[K * B + u % B + 1]]
        want[u] = mine.sum(), (mine == clean).sum()
    return want


@pytest.mark.parametrize("hop", (160, 7))
def test_tally_is_the_count_over_the_returned_labels(ctx, model, coefs, batch, hop):
    flat, offsets = batch
    o = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop)
    want = numpy_stats(o.labels, o.wo)
    print("stats", o.stats.tolist())
    assert np.array_equal(o.stats, want)
    windows = np.diff(o.wo)
    assert np.array_equal(o.stats[K * B:, 1], windows[K * B:])                   # the clean level agrees with itself
    assert (o.stats[windows == 0] == 0).all() and (windows == 0).sum() == 2 * (K + 1)
    quiet = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, want_scores=False, want_labels=False)
    assert np.array_equal(quiet.stats, want)
    assert (bits(quiet.scores) == FILL).all() and (bits(quiet.labels) == FILL).all()


def test_tally_with_both_labels_present(ctx, coefs, batch):
    """The glorot network labels every window of this batch rising, so rising = agree = windows above. Here dense2's bias is
    moved by the median logit difference of the clean windows: about half of them fall on either side, the noise moves some
    across, and the two counts differ from each other and from the window count."""
    flat, offsets = batch
    hop = 7
    w = dict(orc.glorot_weights(7))
    base = sweep(ctx, F2CNNModel(w), coefs, flat, _lib.WAVE_I16, offsets, hop)
    clean = base.scores[base.wo[K * B]:].astype(np.float64)
    w["dense2_b"] = np.array([np.median(np.log(clean[:, 1]) - np.log(clean[:, 0])), 0.0], np.float32)
    o = sweep(ctx, F2CNNModel(w), coefs, flat, _lib.WAVE_I16, offsets, hop)
    windows = np.diff(o.wo)
    print("windows", windows.tolist(), "stats", o.stats.tolist())
    assert 0 < o.stats[K * B + 1, 0] < windows[K * B + 1]                        # the clean 4000-sample row holds both labels
    assert np.array_equal(o.stats, numpy_stats(o.labels, o.wo))
    assert np.array_equal(o.stats[K * B:, 1], windows[K * B:]) and (o.stats[:, 1] <= windows).all()
    assert (o.stats[:K * B, 1] < windows[:K * B]).any()                           # some noisy window changed sides


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["K=0", "snr NULL", "snr nan", "hop=0", "offsets decreasing"])
def test_bad_arguments_leave_the_outputs_alone(ctx, model, coefs, batch, case):
    flat, offsets = batch
    snr, k, hop = np.array(SNR), K, 160
    if case == "K=0":
        k = 0
    elif case == "snr NULL":
        snr = None
    elif case == "snr nan":
        snr, k = np.array([np.nan]), 1
    elif case == "hop=0":
        hop = 0
    else:
        offsets = offsets.copy()
        offsets[2] = offsets[1] - 1
    o = Out(int(batch[1][-1]), 160)
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, snr, k, SEED, o)
    assert rc == _lib.F2_ERR_INVALID, case
    assert o.untouched(), case


def test_no_window_anywhere_still_fills_the_small_outputs(ctx, model, coefs):
    flat, offsets = ragged_waves((1700, 0), seed=50)
    o = Out(1700, 160)
    snr = np.array(SNR)
    o.wo, o.sigma, o.stats = filled((K + 1) * 2 + 1, np.int64), filled((K + 1) * 2, np.float64), filled(((K + 1) * 2, 2), np.int64)
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, snr, K, SEED, o, nbatch=2)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    assert (o.wo == 0).all() and (o.stats == 0).all()
    rms = np.sqrt(np.mean(np.square(flat.astype(np.float64))))
    assert np.allclose(o.sigma, [rms / 10, 0, rms / 10 ** -0.3, 0, 0, 0], rtol=1e-15)
    empty = Out(0, 160)
    empty.wo, empty.sigma, empty.stats = filled(1, np.int64), filled(0, np.float64), filled((0, 2), np.int64)
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, np.zeros(1, np.int64), 160, snr, K, SEED, empty, nbatch=0)
    assert rc == _lib.F2_OK and empty.wo[0] == 0


# ---- 6. Python layer ----------------------------------------------------------------------------------------------------------
def test_evaluate_noise_sweep_writes_a_reproducible_npz(tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    from f2cnn_amd import config
    from f2cnn_amd.scripts.CNN import Evaluating
    monkeypatch.chdir(tmp_path)
    config.write_default()
    m = F2CNNModel(orc.glorot_weights(7))
    wave = orc.synth_utterance(77, 5000).astype(np.int16)
    wav = str(tmp_path / "DR1.FAAA0.SA1.WAV")
    wavfile.write(wav, 16000, wave)
    hop = 160
    res = Evaluating.EvaluateNoiseSweep([wav], [10, -3], seed=11, hop=hop, model=m)[wav]
    out = os.path.join("OutputWavFiles", "addedNoise", "DR1.FAAA0.SA1.sweep.npz")
    first = dict(np.load(out))
    assert sorted(first) == sorted(["snr_db", "sigma", "windows", "rising", "agree", "agreement", "seed", "hop", "labels_0", "labels_1",
                                    "labels_clean"])
    n = len(range(0, 5000 - R * STEP, hop))
    assert first["windows"].tolist() == [n, n, n] and int(first["hop"]) == hop and int(first["seed"]) == 11
    assert np.array_equal(first["agreement"], first["agree"] / first["windows"]) and first["agreement"][K] == 1.0
    assert first["snr_db"].tolist() == [10.0, -3.0] and first["sigma"][K] == 0 and (first["sigma"][:K] > 0).all()
    for k, key in enumerate(("labels_0", "labels_1", "labels_clean")):
        assert first[key].shape == (n,) and first["rising"][k] == first[key].sum()
        assert first["agree"][k] == (first[key] == first["labels_clean"]).sum()
        assert np.array_equal(res[key], first[key])
    _, clean_labels = Evaluating.EvaluateOneWavArray(wave, 16000, model=m, hop=hop)
    assert np.array_equal(first["labels_clean"], clean_labels)
    Evaluating.EvaluateNoiseSweep([wav], [10, -3], seed=11, hop=hop, model=m)
    second = dict(np.load(out))
    for key in first:
        assert np.array_equal(bits(first[key]), bits(second[key])), key
    printed = capsys.readouterr().out
    assert "agreement" in printed and "-3dB" in printed and "clean" in printed
