"""f2_eval_batch_strided: a decision every `hop` samples. Window j of utterance b IS every-sample window j * hop of
f2_eval_batch - same envelope, same window arithmetic, same network - so every comparison with the every-sample calls is
on raw bits, with no tolerance; one check against the oracle chain stands beside them. All through the C ABI via ctypes."""
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
CNN_CHUNK = 16384                                  # windows per chunk (csrc/f2_pipeline.hip)
DIVISORS, OTHERS = (1, 2, 5, 16, 160), (3, 7, 100, 161)
# ragged: one window, short, one CNN chunk of every-sample windows, more than one, no window (n <= 11 * step), empty
LENGTHS = (1761, 4000, 16000, 23456, 1700, 0)


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


def nb_of(n):
    return max(0, n - R * STEP)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def ragged_waves(lengths, seed=40):
    """synthetic utterances; the 4000-sample one is speech-shaped (a syllable rhythm over a noise floor: tests/speechlike.py)"""
    waves = []
    for i, n in enumerate(lengths):
        waves.append(speechlike.make(seed + i, n, "syllables")[0] if n == 4000 else orc.synth_utterance(seed + i, n))
    offsets = np.zeros(len(lengths) + 1, np.int64)
    offsets[1:] = np.cumsum(lengths)
    return np.concatenate(waves).astype(np.int16), offsets


def every_sample(ctx, model, coefs, flat, offsets, lpf, precision):
    B = len(offsets) - 1
    nbs = [nb_of(int(n)) for n in np.diff(offsets)]
    sc = np.empty((sum(nbs), 2), np.float32)
    lb = np.empty(sum(nbs), np.uint8)
    ctx.eval_batch(model.handle(ctx), flat, _lib.WAVE_I16, offsets, coefs, B, C, lpf, 50.0 if lpf else 0.0, precision, RADIUS, STEP,
                   sc, lb, _lib.MEM_HOST)
    return sc, lb, np.concatenate([[0], np.cumsum(nbs)]).astype(np.int64)


def strided(ctx, model, coefs, flat, offsets, lpf, precision, hop, mem=_lib.MEM_HOST, want_scores=True, want_labels=True):
    """-> scores, labels (None where not asked for), window_offsets; outputs pre-filled with 0x5A"""
    B = len(offsets) - 1
    total = sum(_lib.strided_window_count(int(n), RADIUS, STEP, hop) for n in np.diff(offsets))
    sc = np.full((total, 2), np.nan, np.float32)
    sc.view(np.uint8)[...] = 0x5A
    lb = np.full(total, 0x5A, np.uint8)
    cutoff = 50.0 if lpf else 0.0
    if mem == _lib.MEM_HOST:
        wo = ctx.eval_batch_strided(model.handle(ctx), flat, _lib.WAVE_I16, offsets, coefs, B, C, lpf, cutoff, precision, RADIUS, STEP,
                                    hop, sc if want_scores else None, lb if want_labels else None, mem)
    else:
        d_wave, d_sc, d_lb = ctx.malloc(max(flat.nbytes, 8)), ctx.malloc(max(sc.nbytes, 8)), ctx.malloc(max(lb.nbytes, 8))
        try:
            ctx.h2d(d_wave, flat)
            ctx.h2d(d_sc, sc)
            ctx.h2d(d_lb, lb)
            wo = ctx.eval_batch_strided(model.handle(ctx), d_wave, _lib.WAVE_I16, offsets, coefs, B, C, lpf, cutoff, precision,
                                        RADIUS, STEP, hop, d_sc if want_scores else None, d_lb if want_labels else None, mem)
            ctx.synchronize()
            if total:
                ctx.d2h(sc, d_sc)
                ctx.d2h(lb, d_lb)
        finally:
            ctx.synchronize()
            for p in (d_wave, d_sc, d_lb):
                ctx.free(p)
    assert wo[-1] == total
    return (sc if want_scores else None), (lb if want_labels else None), wo


def assert_rows_are_every_sample_rows(sc_h, lb_h, wo, sc_1, lb_1, off_1, hop, lengths):
    assert len(wo) == len(lengths) + 1 and wo[0] == 0
    for b, n in enumerate(lengths):
        nb = nb_of(n)
        assert wo[b + 1] - wo[b] == (nb + hop - 1) // hop, (b, n, hop)
        rows = off_1[b] + np.arange(0, nb, hop)
        if sc_h is not None:
            got, want = sc_h[wo[b]:wo[b + 1]], sc_1[rows]
            assert np.array_equal(bits(got), bits(want)), \
                f"utterance {b} ({n} samples), hop {hop}: scores differ in {np.count_nonzero((got != want).any(axis=1))} of {len(rows)} windows"
        if lb_h is not None:
            assert np.array_equal(lb_h[wo[b]:wo[b + 1]], lb_1[rows]), (b, n, hop)


@pytest.fixture(scope="module")
def ragged(ctx, model, coefs):
    """the ragged batch and its every-sample results per (lpf, precision), computed once"""
    flat, offsets = ragged_waves(LENGTHS)
    cache = {}

    def get(lpf, precision):
        if (lpf, precision) not in cache:
            cache[lpf, precision] = every_sample(ctx, model, coefs, flat, offsets, lpf, precision)
        return cache[lpf, precision]
    return flat, offsets, get


@pytest.mark.parametrize("hop", DIVISORS + OTHERS)
@pytest.mark.parametrize("precision", [_lib.FFT_F32, _lib.FFT_F64], ids=["fft32", "fft64"])
@pytest.mark.parametrize("lpf", [False, True], ids=["nolpf", "lpf50"])
def test_strided_rows_are_the_every_sample_rows(ctx, model, coefs, ragged, lpf, precision, hop):
    """Check 4 of the issue, the main one: raw float32 bits, hop dividing STEP (decimating kernels) and not (per-window kernel)."""
    flat, offsets, get = ragged
    sc_1, lb_1, off_1 = get(lpf, precision)
    sc_h, lb_h, wo = strided(ctx, model, coefs, flat, offsets, lpf, precision, hop)
    assert_rows_are_every_sample_rows(sc_h, lb_h, wo, sc_1, lb_1, off_1, hop, LENGTHS)
    assert sc_h.min() >= 0 and sc_h.max() <= 1 and set(np.unique(lb_h)) <= {0, 1}          # (written: not the fill byte)


@pytest.mark.parametrize("hop", (1, 16, 160, 7))
def test_device_buffers_and_optional_outputs(ctx, model, coefs, ragged, hop):
    flat, offsets, get = ragged
    sc_1, lb_1, off_1 = get(False, _lib.FFT_F32)
    sc_h, lb_h, wo = strided(ctx, model, coefs, flat, offsets, False, _lib.FFT_F32, hop, mem=_lib.MEM_DEVICE)
    assert_rows_are_every_sample_rows(sc_h, lb_h, wo, sc_1, lb_1, off_1, hop, LENGTHS)
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        sc_h, none, wo = strided(ctx, model, coefs, flat, offsets, False, _lib.FFT_F32, hop, mem=mem, want_labels=False)
        assert none is None
        assert_rows_are_every_sample_rows(sc_h, None, wo, sc_1, lb_1, off_1, hop, LENGTHS)
        none, lb_h, wo = strided(ctx, model, coefs, flat, offsets, False, _lib.FFT_F32, hop, mem=mem, want_scores=False)
        assert none is None
        assert_rows_are_every_sample_rows(None, lb_h, wo, sc_1, lb_1, off_1, hop, LENGTHS)
        none, none2, wo = strided(ctx, model, coefs, flat, offsets, False, _lib.FFT_F32, hop, mem=mem, want_scores=False,
                                  want_labels=False)
        assert none is None and none2 is None and wo[-1] == sum((nb_of(n) + hop - 1) // hop for n in LENGTHS)


@pytest.mark.parametrize("rows,channels", [(11, 67), (13, 40)], ids=["11x67", "13x40"])
def test_strided_rows_are_the_every_sample_rows_where_the_channel_tails_run(ctx, rows, channels):
    """The window kernels' partial channel group and their two store forms, on both routes: 67 channels end in a group of 3 and
    take the scalar store tail (67 % 4 != 0), 40 end in a group of 8 and take the float4 stores. STEP = 16 keeps the batch tiny;
    with W = rows * 16 the utterances have 1, 33 (a block of 32 windows and one), 200 (a partial last block), 500 - W (several
    blocks), no window, and no samples. Hops 1, 2 and 16 divide STEP (table-driven kernels), 3 does not (per-window kernel);
    the reference is f2_eval_batch on the same batch, whose utterances of 200 and 500 - W windows take the every-sample blocked
    kernels and the shorter ones the per-window kernel. Raw bits of scores and labels."""
    step, radius, W = 16, (rows - 1) // 2, rows * 16
    assert 2 * radius + 1 == rows
    lengths = (W + 1, W + 33, W + 200, 500, W, 0)
    flat, offsets = ragged_waves(lengths, seed=70)
    B = len(lengths)
    cf = orc.make_erb_filters(16000, orc.centre_freqs(16000, channels, 100))
    h = F2CNNModel.glorot(7, rows, channels).handle(ctx)
    nbs = [max(0, n - W) for n in lengths]
    off_1 = np.concatenate([[0], np.cumsum(nbs)]).astype(np.int64)
    sc_1, lb_1 = np.empty((sum(nbs), 2), np.float32), np.empty(sum(nbs), np.uint8)
    ctx.eval_batch(h, flat, _lib.WAVE_I16, offsets, cf, B, channels, False, 0.0, _lib.FFT_F32, radius, step, sc_1, lb_1, _lib.MEM_HOST)
    for hop in (1, 2, 16, 3):
        counts = [(nb + hop - 1) // hop for nb in nbs]
        assert counts == [_lib.strided_window_count(n, radius, step, hop) for n in lengths]
        sc = np.empty((sum(counts), 2), np.float32)
        sc.view(np.uint8)[...] = 0x5A
        lb = np.full(sum(counts), 0x5A, np.uint8)
        wo = ctx.eval_batch_strided(h, flat, _lib.WAVE_I16, offsets, cf, B, channels, False, 0.0, _lib.FFT_F32, radius, step, hop, sc,
                                    lb, _lib.MEM_HOST)
        assert np.array_equal(wo, np.concatenate([[0], np.cumsum(counts)])), hop
        for b, nb in enumerate(nbs):
            rows_1 = off_1[b] + np.arange(0, nb, hop)
            got, want = sc[wo[b]:wo[b + 1]], sc_1[rows_1]
            assert np.array_equal(bits(got), bits(want)), \
                f"utterance {b} ({lengths[b]} samples), hop {hop}: scores differ in {np.count_nonzero((got != want).any(axis=1))} of {len(rows_1)} windows"
            assert np.array_equal(lb[wo[b]:wo[b + 1]], lb_1[rows_1]), (b, hop)
        assert set(np.unique(lb)) <= {0, 1}                                                    # (written: not the fill byte)


def test_per_window_route_when_the_blocked_kernels_are_switched_off(ctx, model, coefs, ragged):
    """option gather_blocked = 0 sends a hop that divides STEP through the per-window kernel as well: same rows"""
    flat, offsets, get = ragged
    sc_1, lb_1, off_1 = get(False, _lib.FFT_F32)
    with ctx.options(gather_blocked=0):
        sc_h, lb_h, wo = strided(ctx, model, coefs, flat, offsets, False, _lib.FFT_F32, 16)
    assert_rows_are_every_sample_rows(sc_h, lb_h, wo, sc_1, lb_1, off_1, 16, LENGTHS)


def test_windows_only():
    """Check 5 of the issue. The windows of the strided call are not reachable through the ABI: the call keeps them in a device
    scratch buffer between its window stage and the network, and no diagnostic export was added for them. They are compared
    through check 4 only: a window that differed from every-sample window j * hop in one bit of one of its 1408 values would
    have to leave both float32 scores unchanged in all 36 (lpf, precision, hop) cases of that test to go unseen. What the
    every-sample windows themselves are is pinned against orc.eval_input_tensor by tests/test_gpu_windows_cnn.py
    (test_eval_windows_match_the_reference_predict_argument, test_every_sample_windows_blocked_and_per_window_kernels_agree)."""
    exported = [n for n in _lib.SIGNATURES if "strided" in n]
    assert exported == ["f2_eval_batch_strided"]


def test_against_the_oracle_chain_at_one_decision_per_frame(ctx, model, coefs):
    """Check 6: filter_and_envelope -> eval_input_tensor[::hop] -> cnn_forward on a 1 s utterance at hop = 160, with the score
    tolerance of f2_eval_* against the oracle, atol = 5e-4 (tests/test_gpu_windows_cnn.py:308 and :332,
    tests/test_gpu_cli_files.py:113), and its rule for labels (tests/test_gpu_windows_cnn.py:309-315)."""
    hop, N = 160, 16000
    wave = orc.synth_utterance(2028, N)
    offsets = np.array([0, N], np.int64)
    sc, lb, wo = strided(ctx, model, coefs, wave, offsets, False, _lib.FFT_F32, hop)
    assert list(wo) == [0, 89]
    env = orc.filter_and_envelope(wave, coefs, False)
    x = orc.eval_input_tensor(env)[::hop]
    assert x.shape[0] == 89
    w = dict(model.tensors)
    ref = orc.cnn_forward(x, w)
    print("max |score - oracle| =", float(np.abs(sc - ref).max()))
    np.testing.assert_allclose(sc, ref, atol=5e-4)
    differ = np.flatnonzero(lb != orc.labels_from_scores(ref))
    if len(differ):
        r = orc.cnn_forward_referee(x[differ], w)
        assert np.abs(r[:, 1] - r[:, 0]).max() <= 1e-3
    assert len(differ) <= 0.01 * len(lb)


def test_chunks_cross_utterance_boundaries(ctx, model, coefs):
    """Check 7: 40 x 1 s at hop = 16 is 35 600 windows - three chunks; utterance 18 (windows 16 020 .. 16 909) straddles the
    first chunk boundary at 16 384, utterance 36 the second at 32 768, and every chunk holds many utterances. The first, the
    last and the boundary utterances against f2_eval_utterance of each alone."""
    hop, N, B = 16, 16000, 40
    per = (nb_of(N) + hop - 1) // hop
    assert per == 890 and B * per > 2 * CNN_CHUNK
    straddle = [b for b in range(B) if b * per // CNN_CHUNK != ((b + 1) * per - 1) // CNN_CHUNK]
    assert straddle == [18, 36]
    waves = [orc.synth_utterance(700 + b, N) for b in range(B)]
    offsets = np.arange(B + 1, dtype=np.int64) * N
    sc, lb, wo = strided(ctx, model, coefs, np.concatenate(waves), offsets, False, _lib.FFT_F32, hop)
    assert np.array_equal(wo, np.arange(B + 1) * per)
    for b in sorted({0, B - 1, *straddle, straddle[0] - 1, straddle[0] + 1}):
        s1 = np.empty((nb_of(N), 2), np.float32)
        l1 = np.empty(nb_of(N), np.uint8)
        got = ctx.eval_utterance(model.handle(ctx), waves[b], _lib.WAVE_I16, N, coefs, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, None,
                                 s1, l1, _lib.MEM_HOST)
        assert got == nb_of(N)
        assert np.array_equal(bits(sc[wo[b]:wo[b + 1]]), bits(s1[::hop])), f"utterance {b}"
        assert np.array_equal(lb[wo[b]:wo[b + 1]], l1[::hop]), f"utterance {b}"


def launches(ctx, model, coefs, flat, offsets, hop):
    ctx.prof_enable(True)
    try:
        strided(ctx, model, coefs, flat, offsets, False, _lib.FFT_F32, hop)
        got = {}
        for k, name in ((2, "gather"), (3, "cnn")):                 # F2_K_GATHER, F2_K_CNN (include/f2cnn_hip.h)
            n, ms = ctypes.c_int(), ctypes.c_float()
            assert ctx.lib.f2_prof_get(ctx.handle, k, ctypes.byref(n), ctypes.byref(ms)) == _lib.F2_OK
            got[name] = n.value
        return got
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("hop", (160, 100), ids=["decimating", "per_window"])
def test_launches_do_not_scale_with_the_batch(ctx, model, coefs, hop):
    """Check 8: 64 utterances of 2000 samples (two or three windows each: one chunk) launch what one utterance whose windows fit one
    chunk launches - one window-stage group and, for the network, one convolution group and one dense group."""
    B, n = 64, 2000
    flat = np.concatenate([orc.synth_utterance(800 + b, n) for b in range(B)])
    many = launches(ctx, model, coefs, flat, np.arange(B + 1, dtype=np.int64) * n, hop)
    one = launches(ctx, model, coefs, orc.synth_utterance(900, 16000), np.array([0, 16000], np.int64), hop)
    PER_CHUNK = {"gather": 1, "cnn": 2}
    assert one == PER_CHUNK
    assert many == PER_CHUNK
    assert many["gather"] + many["cnn"] < B // 8


def call_raw(ctx, model, coefs, flat, offsets, hop, n_rows):
    sc, lb = np.zeros((n_rows, 2), np.float32), np.zeros(n_rows, np.uint8)
    wo = np.full(len(offsets), -1, np.int64)
    rc = ctx.lib.f2_eval_batch_strided(ctx.handle, model.handle(ctx), flat.ctypes.data, _lib.WAVE_I16, offsets.ctypes.data,
                                       coefs.ctypes.data, len(offsets) - 1, C, 0, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, sc.ctypes.data,
                                       lb.ctypes.data, wo.ctypes.data, _lib.MEM_HOST)
    return rc, sc, lb, wo


@pytest.mark.parametrize("hop", (0, -1))
def test_hop_below_one_is_refused_before_anything_is_launched(ctx, model, coefs, hop):
    flat, offsets = ragged_waves((4000, 2000))
    ctx.prof_enable(True)
    try:
        rc, _, _, _ = call_raw(ctx, model, coefs, flat, offsets, hop, 6000)
        assert rc == _lib.F2_ERR_INVALID
        assert "hop" in ctx.lib.f2_last_error(ctx.handle).decode()
        assert ctx.prof_get() == {}
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("hop", (16, 7))
def test_only_evaluated_windows_raise_nonpositive(ctx, model, coefs, hop):
    """Check 9: an all-zero utterance (its envelope is zero) fails the call when it is long enough to have windows, and does not
    when it has none; the other utterances' rows are then the every-sample rows."""
    lens = (4000, 3000, 2500)
    parts = [orc.synth_utterance(60, lens[0]), np.zeros(lens[1], np.int16), orc.synth_utterance(61, lens[2])]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = sum((nb_of(n) + hop - 1) // hop for n in lens)
    rc, _, _, _ = call_raw(ctx, model, coefs, np.concatenate(parts), offsets, hop, total)
    assert rc == _lib.F2_ERR_NONPOSITIVE
    lens = (4000, R * STEP, 2500)                        # the silent utterance cut to 11 * step samples: no window reads it
    parts[1] = np.zeros(lens[1], np.int16)
    flat = np.concatenate(parts)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = sum((nb_of(n) + hop - 1) // hop for n in lens)
    rc, sc, lb, wo = call_raw(ctx, model, coefs, flat, offsets, hop, total)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    assert wo[1] == wo[2]
    for b in (0, 2):
        s1 = np.empty((nb_of(lens[b]), 2), np.float32)
        l1 = np.empty(nb_of(lens[b]), np.uint8)
        ctx.eval_utterance(model.handle(ctx), parts[b], _lib.WAVE_I16, lens[b], coefs, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, None,
                           s1, l1, _lib.MEM_HOST)
        assert np.array_equal(bits(sc[wo[b]:wo[b + 1]]), bits(s1[::hop])) and np.array_equal(lb[wo[b]:wo[b + 1]], l1[::hop])


def test_python_and_cli_write_hop_and_timepoints(tmp_path, monkeypatch, capsys):
    """Check 10: EvaluateWavArrays(hop=160) and `cnn eval --file X.WAV --hop frame` against the same calls without a hop."""
    from f2cnn_amd import cli, config, wavio
    from f2cnn_amd.scripts.CNN import Evaluating
    monkeypatch.chdir(tmp_path)
    config.write_default()
    m = F2CNNModel(orc.glorot_weights(7))
    waves = [orc.synth_utterance(900 + i, n) for i, n in enumerate((3000, 1700, 16000, 1761))]
    full = Evaluating.EvaluateWavArrays(waves, 16000, model=m)
    hopped = Evaluating.EvaluateWavArrays(waves, 16000, model=m, hop=160)
    assert [len(l) for _, l in hopped] == [8, 0, 89, 1]
    for (s1, l1), (sh, lh) in zip(full, hopped):
        assert np.array_equal(bits(sh), bits(s1[::160])) and np.array_equal(lh, l1[::160])
    sh, lh = Evaluating.EvaluateOneWavArray(waves[0], 16000, model=m, hop=7)
    assert np.array_equal(bits(sh), bits(full[0][0][::7])) and np.array_equal(lh, full[0][1][::7])
    with pytest.raises(ValueError):
        Evaluating.EvaluateOneWavArray(np.zeros(4000, np.int16), 16000, model=m, hop=160)       # normalizeInput's error

    os.makedirs(os.path.join("resources", "f2cnn", "TEST"))
    wav = os.path.join("resources", "f2cnn", "TEST", "DR1.FAAA0.SA1.WAV")
    wavio.write_sphere(wav, 16000, orc.synth_utterance(77, 5000))
    m.save("last_trained_model.npz")
    out = os.path.splitext(wav)[0] + ".F2CNN.npz"
    assert cli.main(["cnn", "eval", "--file", wav, "--model", "last_trained_model.npz"]) == 0
    plain = dict(np.load(out))
    assert sorted(plain) == ["labels", "scores"] and plain["labels"].shape == (5000 - 1760,)
    assert cli.main(["cnn", "eval", "--file", wav, "--model", "last_trained_model.npz", "--hop", "frame"]) == 0
    res = dict(np.load(out))
    assert sorted(res) == ["hop", "labels", "scores", "timepoints"]
    assert int(res["hop"]) == 160 and res["timepoints"].dtype == np.int64
    n = len(range(0, 5000 - 1760, 160))
    assert res["scores"].shape == (n, 2) and res["labels"].shape == (n,) and res["timepoints"].shape == (n,)
    assert np.array_equal(res["timepoints"], 800 + 160 * np.arange(n))
    assert np.array_equal(bits(res["scores"]), bits(plain["scores"][::160])) and np.array_equal(res["labels"], plain["labels"][::160])
    # evalrand: the group of files in one strided call
    assert cli.main(["cnn", "evalrand", "--model", "last_trained_model.npz", "--hop", "16"]) == 0
    res16 = dict(np.load(out))
    assert int(res16["hop"]) == 16 and np.array_equal(bits(res16["scores"]), bits(plain["scores"][::16]))
    assert np.array_equal(res16["timepoints"], 800 + 16 * np.arange(len(res16["labels"])))
    capsys.readouterr()
