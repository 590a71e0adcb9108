"""f2_eval_cutoff_sweep: a ragged batch at K envelope cutoffs and unfiltered in one device pass. The three bit-for-bit statements
of the header - the unfiltered level is f2_eval_batch_strided(lpf = 0), the levels are f2_lowpass_levels of the unfiltered one,
every level's scores are f2_cnn_forward of f2_gather_windows of that level - the levels against the oracle and against the
library's own lpf = 1 route, the tally against counts made from the returned labels, the argument errors. The batch of
tests/test_gpu_noise_sweep.py, through the C ABI via ctypes."""
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
CUTOFFS = (5.0, 50.0)
K = len(CUTOFFS)
U = (K + 1) * B
HOPS = (16, 160)
TOL = 1e-5           # per-channel max-norm against the oracle, relative: the project's bar (tests/test_gpu_lowpass_scan.py)
TOL_ROUTES = 4e-6    # between two routes of the library (the same file)
FILL = 0x5A


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
    """as tests/test_gpu_noise_sweep.py builds its batch: the 4000-sample utterance is speech-shaped"""
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


def n_windows(hop, levels=K + 1, lengths=LENGTHS):
    return levels * sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in lengths)


class Out:
    """every output of one call, pre-filled with 0x5A"""

    def __init__(self, total, hop, levels=K + 1, nbatch=B, lengths=LENGTHS, env=True):
        self.env = filled(levels * C * total if env else 0, np.float64)
        self.scores = filled((n_windows(hop, levels, lengths), 2), np.float32)
        self.labels = filled(n_windows(hop, levels, lengths), np.uint8)
        self.wo = filled(levels * nbatch + 1, np.int64)
        self.stats = filled((levels * nbatch, 2), np.int64)

    def untouched(self):
        return all((bits(a) == FILL).all() for a in (self.env, self.scores, self.labels, self.wo, self.stats))


def raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, cut, k, o, want_env=True, want_scores=True, want_labels=True, nbatch=B,
              nchan=C, mem_space=_lib.MEM_HOST, radius=RADIUS, fft=_lib.FFT_F32, handle=True):
    p = lambda a: None if a is None else a.ctypes.data
    return ctx.lib.f2_eval_cutoff_sweep(ctx.handle, model.handle(ctx) if handle else None, p(wave), dtype, p(offsets), p(coefs), nbatch,
                                        nchan, fft, radius, STEP, hop, p(cut), k, p(o.env) if want_env else None,
                                        p(o.scores) if want_scores else None, p(o.labels) if want_labels else None, p(o.wo),
                                        p(o.stats), mem_space)


def sweep(ctx, model, coefs, wave, dtype, offsets, hop, **kw):
    o = Out(int(offsets[-1]), hop)
    rc = raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, np.array(CUTOFFS), K, o, **kw)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return o


@pytest.fixture(scope="module")
def sweeps(ctx, model, coefs, batch):
    """the int16 batch at both hops: shared by the tests that only read them"""
    flat, offsets = batch
    return {hop: sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop) for hop in HOPS}


def level_blocks(o, offsets, l):
    """the (C, n_b) envelope matrices of level l"""
    total = int(offsets[-1])
    lev = o.env.reshape(K + 1, C * total)[l]
    return [lev[C * offsets[b]:C * offsets[b + 1]].reshape(C, -1) for b in range(B)]


# ---- 1. the contract: no tolerance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", HOPS)
def test_unfiltered_level_is_the_strided_call(ctx, model, coefs, batch, sweeps, hop):
    flat, offsets = batch
    o = sweeps[hop]
    n = n_windows(hop, 1)
    sc, lb = filled((n, 2), np.float32), filled(n, np.uint8)
    wo = ctx.eval_batch_strided(model.handle(ctx), flat, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop,
                                sc, lb, _lib.MEM_HOST)
    assert n > 0 and np.array_equal(o.wo[K * B:] - o.wo[K * B], wo)
    assert np.array_equal(bits(o.scores[o.wo[K * B]:]), bits(sc))
    assert np.array_equal(o.labels[o.wo[K * B]:], lb) and set(np.unique(o.labels)) <= {0, 1}


def test_levels_are_lowpass_levels_of_the_unfiltered_block(ctx, batch, sweeps):
    _, offsets = batch
    o = sweeps[160]
    total = int(offsets[-1])
    own = np.ascontiguousarray(o.env.reshape(K + 1, C * total)[K])
    again = filled((K + 1) * C * total, np.float64)
    ctx.lowpass_levels(own, offsets, B, C, CUTOFFS, again, _lib.MEM_HOST)
    assert np.array_equal(bits(again), bits(o.env))
    assert np.array_equal(bits(sweeps[16].env), bits(o.env))                     # the hop does not enter


@pytest.mark.parametrize("hop", HOPS)
def test_every_levels_scores_are_the_network_on_its_gathered_windows(ctx, model, batch, sweeps, hop):
    _, offsets = batch
    o = sweeps[hop]
    for l in range(K + 1):
        for b, env in enumerate(level_blocks(o, offsets, l)):
            u = l * B + b
            n = int(o.wo[u + 1] - o.wo[u])
            assert n == _lib.strided_window_count(LENGTHS[b], RADIUS, STEP, hop)
            if n == 0:
                continue
            centers = (RADIUS * STEP + hop * np.arange(n)).astype(np.int64)
            win = np.empty((n, R, C), np.float32)
            ctx.gather_windows(np.ascontiguousarray(env), C, LENGTHS[b], centers, n, RADIUS, STEP, True, win, _lib.MEM_HOST)
            sc, lb = np.empty((n, 2), np.float32), np.empty(n, np.uint8)
            ctx.cnn_forward(model.handle(ctx), win, n, sc, lb, _lib.MEM_HOST)
            assert np.array_equal(bits(o.scores[o.wo[u]:o.wo[u + 1]]), bits(sc)), (l, b)
            assert np.array_equal(o.labels[o.wo[u]:o.wo[u + 1]], lb), (l, b)


# ---- 2. the levels against the oracle and the lpf = 1 route -------------------------------------------------------------------------
def chan_relerr(a, b):
    return float((np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max())


def test_levels_against_the_oracle_and_the_lpf_route(ctx, coefs, batch, sweeps):
    flat, offsets = batch
    o = sweeps[160]
    total = int(offsets[-1])
    for l, cutoff in enumerate(CUTOFFS):
        route = np.full(C * total, np.nan)
        with ctx.options(spectral=0):
            ctx.filterbank_envelope_fused(flat, _lib.WAVE_I16, offsets, coefs, B, C, True, cutoff, _lib.FFT_F32, route, None, _lib.MEM_HOST)
        for b, got in enumerate(level_blocks(o, offsets, l)):
            if LENGTHS[b] == 0:
                continue
            want = orc.filter_and_envelope(flat[offsets[b]:offsets[b + 1]], coefs, True, cutoff)
            lib = route[C * offsets[b]:C * offsets[b + 1]].reshape(C, -1)
            e_ref, e_route = chan_relerr(got, want), chan_relerr(got, lib)
            print(f"cutoff {cutoff} utterance {b}: oracle {e_ref:.3g} lpf route {e_route:.3g}")
            assert e_ref <= TOL, (cutoff, b)
            assert e_route <= TOL_ROUTES, (cutoff, b)
    for b, got in enumerate(level_blocks(o, offsets, K)):                        # the unfiltered level
        if LENGTHS[b]:
            assert chan_relerr(got, orc.filter_and_envelope(flat[offsets[b]:offsets[b + 1]], coefs, False)) <= TOL


# ---- 3. tally, window offsets -------------------------------------------------------------------------------------------------------
def numpy_stats(labels, wo):
    want = np.zeros((U, 2), np.int64)
    for u in range(U):
        mine = labels[wo[u]:wo[u + 1]]
        clean = labels[wo[K * B + u % B]:wo[K * B + u % B + 1]]
        want[u] = mine.sum(), (mine == clean).sum()
    return want


@pytest.mark.parametrize("hop", HOPS)
def test_tally_and_window_offsets(ctx, model, coefs, batch, sweeps, hop):
    flat, offsets = batch
    o = sweeps[hop]
    per = [_lib.strided_window_count(n, RADIUS, STEP, hop) for n in LENGTHS] * (K + 1)
    assert np.array_equal(o.wo, np.concatenate([[0], np.cumsum(per)]))
    want = numpy_stats(o.labels, o.wo)
    print("stats", o.stats.tolist())
    assert np.array_equal(o.stats, want)
    windows = np.diff(o.wo)
    assert np.array_equal(o.stats[K * B:, 1], windows[K * B:])                   # the unfiltered level agrees with itself
    quiet = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, want_env=False, want_scores=False, want_labels=False)
    assert np.array_equal(quiet.stats, want) and np.array_equal(quiet.wo, o.wo)
    assert all((bits(a) == FILL).all() for a in (quiet.env, quiet.scores, quiet.labels))


def test_tally_with_both_labels_present(ctx, coefs, batch, sweeps):
    """The glorot network labels every window of this batch rising. Here dense2's bias is moved by the median logit difference
    of the unfiltered windows: about half of them fall on either side and the low-pass moves some across."""
    flat, offsets = batch
    hop = 16
    base = sweeps[hop]
    w = dict(orc.glorot_weights(7))
    clean = base.scores[base.wo[K * B]:].astype(np.float64)
    w["dense2_b"] = np.array([np.median(np.log(clean[:, 1]) - np.log(clean[:, 0])), 0.0], np.float32)
    o = sweep(ctx, F2CNNModel(w), coefs, flat, _lib.WAVE_I16, offsets, hop)
    windows = np.diff(o.wo)
    print("windows", windows.tolist(), "stats", o.stats.tolist())
    assert 0 < o.stats[K * B + 1, 0] < windows[K * B + 1]
    assert np.array_equal(o.stats, numpy_stats(o.labels, o.wo))
    assert np.array_equal(o.stats[K * B:, 1], windows[K * B:]) and (o.stats[:, 1] <= windows).all()


def test_float64_waves_and_a_second_call_give_the_same_bits(ctx, model, coefs, batch, sweeps):
    flat, offsets = batch
    o = sweep(ctx, model, coefs, flat.astype(np.float64), _lib.WAVE_F64, offsets, 160)
    for name in ("env", "scores", "labels", "wo", "stats"):
        assert np.array_equal(bits(getattr(o, name)), bits(getattr(sweeps[160], name))), name


# ---- 4. errors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["K=0", "K=65", "cutoffs NULL", "cutoff nan", "cutoff inf", "cutoff 0", "cutoff 8000", "cutoff -1",
                                  "hop=0", "offsets decreasing", "offsets[0]=1", "offsets NULL", "wave NULL", "coefs NULL", "cnn NULL",
                                  "wave_dtype", "fft_precision", "mem_space", "mem_space async", "C=0", "C=64", "radius=4", "B<0"])
def test_bad_arguments_leave_the_outputs_alone(ctx, model, coefs, batch, case):
    flat, offsets = batch
    cut, k, hop, want = np.array(CUTOFFS), K, 160, _lib.F2_ERR_INVALID
    kw = {}
    wave, dtype, co = flat, _lib.WAVE_I16, coefs
    if case == "K=0":
        k = 0
    elif case == "K=65":
        cut, k, want = np.full(65, 50.0), 65, _lib.F2_ERR_UNSUPPORTED
    elif case == "cutoffs NULL":
        cut = None
    elif case.startswith("cutoff "):
        cut[1] = {"nan": np.nan, "inf": np.inf, "0": 0.0, "8000": 8000.0, "-1": -1.0}[case.split()[1]]
    elif case == "hop=0":
        hop = 0
    elif case == "offsets decreasing":
        offsets = offsets.copy()
        offsets[2] = offsets[1] - 1
    elif case == "offsets[0]=1":
        offsets = offsets.copy()
        offsets[0] = 1
    elif case == "offsets NULL":
        offsets = None
    elif case == "wave NULL":
        wave = None
    elif case == "coefs NULL":
        co = None
    elif case == "cnn NULL":
        kw["handle"] = False
    elif case == "wave_dtype":
        dtype = 9
    elif case == "fft_precision":
        kw["fft"] = 9
    elif case == "mem_space":
        kw["mem_space"] = 7
    elif case == "mem_space async":
        kw["mem_space"] = _lib.MEM_HOST_ASYNC
    elif case == "C=0":
        kw["nchan"] = 0
    elif case == "C=64":
        kw["nchan"] = 64                     # the network was built for 128 channels
    elif case == "radius=4":
        kw["radius"] = 4                     # ... and 11 rows
    else:
        kw["nbatch"] = -1
    o = Out(int(batch[1][-1]), 160, levels=max(k, K) + 1, env=k <= K)           # (66 levels of envelopes: not worth 500 MB)
    rc = raw_sweep(ctx, model, co, wave, dtype, offsets, hop, cut, k, o, want_env=k <= K, **kw)
    assert rc == want, case
    assert o.untouched(), case


def test_no_window_anywhere_and_the_empty_batch(ctx, model, coefs):
    lengths = (1700, 0)
    flat, offsets = ragged_waves(lengths, seed=50)
    o = Out(1700, 160, nbatch=2, lengths=lengths)
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, np.array(CUTOFFS), K, o, nbatch=2)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    assert (o.wo == 0).all() and (o.stats == 0).all()
    env = o.env.reshape(K + 1, C, 1700)                                           # the levels are still made
    assert np.isfinite(env).all() and (env[K] >= 0).all() and env[K].max() > 0
    empty = Out(0, 160, nbatch=0, lengths=())
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, np.zeros(1, np.int64), 160, np.array(CUTOFFS), K, empty, nbatch=0)
    assert rc == _lib.F2_OK and empty.wo[0] == 0
    zero = Out(0, 160, nbatch=2, lengths=(0, 0))
    rc = raw_sweep(ctx, model, coefs, None, _lib.WAVE_I16, np.zeros(3, np.int64), 160, np.array(CUTOFFS), K, zero, nbatch=2)
    assert rc == _lib.F2_OK and (zero.wo == 0).all() and (zero.stats == 0).all()


# ---- 5. Python layer ------------------------------------------------------------------------------------------------------------------
def test_evaluate_cutoff_sweep_writes_a_reproducible_npz(tmp_path, monkeypatch, capsys):
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
    res = Evaluating.EvaluateCutoffSweep([wav], [5, 50], hop=hop, model=m)[wav]
    first = dict(np.load(str(tmp_path / "DR1.FAAA0.SA1.lpfsweep.npz")))
    assert sorted(first) == sorted(["cutoff_hz", "windows", "rising", "agree", "agreement", "hop", "timepoints", "scores", "labels_0",
                                    "labels_1", "labels_nolpf"])
    n = len(range(0, 5000 - R * STEP, hop))
    assert first["windows"].tolist() == [n, n, n] and int(first["hop"]) == hop and first["scores"].shape == (K + 1, n, 2)
    assert first["cutoff_hz"].tolist() == [5.0, 50.0] and first["timepoints"].shape == (n,)
    assert np.array_equal(first["agreement"], first["agree"] / first["windows"]) and first["agreement"][K] == 1.0
    for k, key in enumerate(("labels_0", "labels_1", "labels_nolpf")):
        assert first[key].shape == (n,) and first["rising"][k] == first[key].sum()
        assert first["agree"][k] == (first[key] == first["labels_nolpf"]).sum()
        assert np.array_equal(res[key], first[key])
    _, nolpf_labels = Evaluating.EvaluateOneWavArray(wave, 16000, model=m, hop=hop, LPF=False)
    assert np.array_equal(first["labels_nolpf"], nolpf_labels)
    _, lpf_labels = Evaluating.EvaluateOneWavArray(wave, 16000, model=m, hop=hop, LPF=True, CUTOFF=50)
    assert (first["labels_1"] == lpf_labels).mean() > 0.9                         # the --lpf route, float32 low-pass
    printed = capsys.readouterr().out
    assert "agreement" in printed and "50Hz" in printed and "nolpf" in printed
