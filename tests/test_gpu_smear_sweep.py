"""f2_eval_smear_sweep: a ragged batch at K spectral resolutions and sharp in one device pass. The three bit-for-bit statements of
the header - the sharp level is f2_eval_batch_strided with the same lpf, the levels are f2_channel_mix_levels of the sharp one,
every level's scores are f2_cnn_forward of f2_gather_windows of that level - the tally against counts made from the returned
labels, identity matrices against the sharp level, the outputs left out one at a time, the empty calls and the argument errors in
the header's order. 16 channels; through the C ABI via ctypes."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib, smear
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

C, RADIUS, STEP = 16, 5, 160
R = 2 * RADIUS + 1
LENGTHS = (1761, 4000, 1700, 4999)       # one window, a few hundred, none (n <= 11 * step), a few hundred of an odd length
B = len(LENGTHS)
FREQS = filters.centre_freqs(16000, C, 100)
SPACING = smear.channel_spacing(FREQS)
MIX = np.stack([smear.SmearMatrix(FREQS, 2.0), smear.BandMatrix(C, 4), smear.BandMatrix(C, C), smear.SmearMatrix(FREQS, SPACING / 5)])
IDENTITIES = (2, 3)
K = len(MIX)
U = (K + 1) * B
# hop, lpf, dtype of the wave: both hops, the low-pass off and on at 50 Hz, int16 and float64
CONFIGS = [(160, 0, _lib.WAVE_I16), (7, 1, _lib.WAVE_I16), (7, 0, _lib.WAVE_F64), (160, 1, _lib.WAVE_F64)]
CONFIG_IDS = ["hop160-i16", "hop7-lpf-i16", "hop7-f64", "hop160-lpf-f64"]
CUTOFF = 50.0
FILL = 0x5A


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return np.ascontiguousarray(filters.make_erb_filters(16000, FREQS))


@pytest.fixture(scope="module")
def model():
    return F2CNNModel.glorot(7, R, C)


def ragged_waves(lengths, seed=60):
    offsets = np.zeros(len(lengths) + 1, np.int64)
    offsets[1:] = np.cumsum(lengths)
    return np.concatenate([orc.synth_utterance(seed + i, n) for i, n in enumerate(lengths)]).astype(np.int16), offsets


@pytest.fixture(scope="module")
def batch():
    flat, offsets = ragged_waves(LENGTHS)
    flat.setflags(write=False)
    return flat, offsets


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


def raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, mix, k, o, lpf=0, want=("env", "scores", "labels", "wo", "stats"), nbatch=B,
              nchan=C, mem_space=_lib.MEM_HOST, radius=RADIUS, fft=_lib.FFT_F32, handle=True, cutoff=None):
    p = lambda a: None if a is None else a.ctypes.data
    give = lambda name: p(getattr(o, name)) if name in want else None
    return ctx.lib.f2_eval_smear_sweep(ctx.handle, model.handle(ctx) if handle else None, p(wave), dtype, p(offsets), p(coefs), nbatch,
                                       nchan, lpf, (CUTOFF if lpf else 0.0) if cutoff is None else cutoff, fft, radius, STEP, hop, p(mix), k,
                                       give("env"), give("scores"), give("labels"), give("wo"), give("stats"), mem_space)


def sweep(ctx, model, coefs, wave, dtype, offsets, hop, lpf, mix=MIX, **kw):
    o = Out(int(offsets[-1]), hop, levels=len(mix) + 1)
    rc = raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, np.ascontiguousarray(mix), len(mix), o, lpf=lpf, **kw)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return o


def wave_as(flat, dtype):
    return flat if dtype == _lib.WAVE_I16 else flat.astype(np.float64)


@pytest.fixture(scope="module")
def sweeps(ctx, model, coefs, batch):
    """the batch under every configuration: shared by the tests that only read them"""
    flat, offsets = batch
    return {cfg: sweep(ctx, model, coefs, wave_as(flat, cfg[2]), cfg[2], offsets, cfg[0], cfg[1]) for cfg in CONFIGS}


def level_blocks(o, offsets, l):
    """the (C, n_b) envelope matrices of level l"""
    total = int(offsets[-1])
    lev = o.env.reshape(K + 1, C * total)[l]
    return [lev[C * offsets[b]:C * offsets[b + 1]].reshape(C, -1) for b in range(B)]


# ---- 1. the contract: no tolerance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_sharp_level_is_the_strided_call(ctx, model, coefs, batch, sweeps, cfg):
    hop, lpf, dtype = cfg
    flat, offsets = batch
    o = sweeps[cfg]
    n = n_windows(hop, 1)
    sc, lb = filled((n, 2), np.float32), filled(n, np.uint8)
    wo = ctx.eval_batch_strided(model.handle(ctx), wave_as(flat, dtype), dtype, offsets, coefs, B, C, bool(lpf), CUTOFF if lpf else 0.0,
                                _lib.FFT_F32, RADIUS, STEP, hop, sc, lb, _lib.MEM_HOST)
    assert n > 0 and np.array_equal(o.wo[K * B:] - o.wo[K * B], wo)
    assert np.array_equal(bits(o.scores[o.wo[K * B]:]), bits(sc))
    assert np.array_equal(o.labels[o.wo[K * B]:], lb) and set(np.unique(o.labels)) <= {0, 1}


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_levels_are_channel_mix_levels_of_the_sharp_block(ctx, batch, sweeps, cfg):
    _, offsets = batch
    o = sweeps[cfg]
    total = int(offsets[-1])
    own = np.ascontiguousarray(o.env.reshape(K + 1, C * total)[K])
    assert np.isfinite(own).all() and own.max() > 0
    again = filled((K + 1) * C * total, np.float64)
    ctx.channel_mix_levels(own, offsets, B, C, MIX, again, _lib.MEM_HOST)
    assert np.array_equal(bits(again), bits(o.env))
    for l in IDENTITIES:                                                          # an identity level is the sharp one (no -0.0 here)
        assert np.array_equal(bits(o.env.reshape(K + 1, -1)[l]), bits(own))


def test_the_hop_does_not_enter_the_levels(sweeps):
    a, b = sweeps[(160, 0, _lib.WAVE_I16)], sweeps[(7, 0, _lib.WAVE_F64)]           # equal values as int16 and float64, another hop
    assert np.array_equal(bits(a.env), bits(b.env))


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_every_levels_scores_are_the_network_on_its_gathered_windows(ctx, model, batch, sweeps, cfg):
    hop = cfg[0]
    _, offsets = batch
    o = sweeps[cfg]
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


# ---- 2. tally, window offsets, identity levels ----------------------------------------------------------------------------------------
def numpy_stats(labels, wo, levels=K + 1):
    want = np.zeros((levels * B, 2), np.int64)
    for u in range(levels * B):
        mine = labels[wo[u]:wo[u + 1]]
        sharp = labels[wo[(levels - 1) * B + u % B]:wo[(levels - 1) * B + u % B + 1]]
        want[u] = mine.sum(), (mine == sharp).sum()
    return want


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_tally_window_offsets_and_identity_levels(sweeps, cfg):
    hop = cfg[0]
    o = sweeps[cfg]
    per = [_lib.strided_window_count(n, RADIUS, STEP, hop) for n in LENGTHS] * (K + 1)
    assert np.array_equal(o.wo, np.concatenate([[0], np.cumsum(per)]))
    want = numpy_stats(o.labels, o.wo)
    print("stats", o.stats.tolist())
    assert np.array_equal(o.stats, want)
    windows = np.diff(o.wo)
    assert np.array_equal(o.stats[K * B:, 1], windows[K * B:])                   # the sharp level agrees with itself
    for l in IDENTITIES:                                                          # and so does a level with the identity matrix
        rows = slice(l * B, (l + 1) * B)
        assert np.array_equal(o.stats[rows, 1], windows[rows]) and np.array_equal(o.stats[rows], o.stats[K * B:])
        assert np.array_equal(o.labels[o.wo[l * B]:o.wo[(l + 1) * B]], o.labels[o.wo[K * B]:])
        assert np.array_equal(bits(o.scores[o.wo[l * B]:o.wo[(l + 1) * B]]), bits(o.scores[o.wo[K * B]:]))


def test_tally_with_both_labels_present(ctx, coefs, batch, sweeps):
    """dense2's bias is moved by the median logit difference of the sharp windows: about half of them fall on either side and the
    smearing moves some across"""
    flat, offsets = batch
    cfg = CONFIGS[1]
    base = sweeps[cfg]
    w = dict(F2CNNModel.glorot(7, R, C).tensors)
    sharp = base.scores[base.wo[K * B]:].astype(np.float64)
    w["dense2_b"] = np.array([np.median(np.log(sharp[:, 1]) - np.log(sharp[:, 0])), 0.0], np.float32)
    o = sweep(ctx, F2CNNModel(w, R, C), coefs, flat, _lib.WAVE_I16, offsets, cfg[0], cfg[1])
    windows = np.diff(o.wo)
    print("windows", windows.tolist(), "stats", o.stats.tolist())
    assert 0 < o.stats[K * B + 1, 0] < windows[K * B + 1]
    assert np.array_equal(o.stats, numpy_stats(o.labels, o.wo))
    assert np.array_equal(o.stats[K * B:, 1], windows[K * B:]) and (o.stats[:, 1] <= windows).all()


@pytest.mark.parametrize("left_out", ["env", "scores", "labels", "wo", "stats"])
def test_every_output_can_be_left_out(ctx, model, coefs, batch, sweeps, left_out):
    flat, offsets = batch
    cfg = CONFIGS[0]
    ref = sweeps[cfg]
    want = tuple(n for n in ("env", "scores", "labels", "wo", "stats") if n != left_out)
    o = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, cfg[0], cfg[1], want=want)
    for name in ("env", "scores", "labels", "wo", "stats"):
        if name == left_out:
            assert (bits(getattr(o, name)) == FILL).all()
        else:
            assert np.array_equal(bits(getattr(o, name)), bits(getattr(ref, name))), name


def test_all_outputs_left_out_and_a_second_call(ctx, model, coefs, batch, sweeps):
    flat, offsets = batch
    cfg = CONFIGS[0]
    quiet = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, cfg[0], cfg[1], want=())
    assert quiet.untouched()
    again = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, cfg[0], cfg[1])
    for name in ("env", "scores", "labels", "wo", "stats"):
        assert np.array_equal(bits(getattr(again, name)), bits(getattr(sweeps[cfg], name))), name


# ---- 3. empty calls, a zero row, errors -------------------------------------------------------------------------------------------------
def test_no_window_anywhere_and_the_empty_batch(ctx, model, coefs):
    lengths = (1700, 0)
    flat, offsets = ragged_waves(lengths, seed=50)
    mix = np.ascontiguousarray(MIX)
    o = Out(1700, 160, nbatch=2, lengths=lengths)
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, mix, K, o, nbatch=2)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    assert (o.wo == 0).all() and (o.stats == 0).all()
    env = o.env.reshape(K + 1, C, 1700)                                           # the levels are still made
    assert np.isfinite(env).all() and (env[K] >= 0).all() and env[K].max() > 0
    assert np.array_equal(bits(env[IDENTITIES[0]]), bits(env[K]))
    empty = Out(0, 160, nbatch=0, lengths=())
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, np.zeros(1, np.int64), 160, mix, K, empty, nbatch=0)
    assert rc == _lib.F2_OK and empty.wo[0] == 0
    zero = Out(0, 160, nbatch=2, lengths=(0, 0))
    rc = raw_sweep(ctx, model, coefs, None, _lib.WAVE_I16, np.zeros(3, np.int64), 160, mix, K, zero, nbatch=2)
    assert rc == _lib.F2_OK and (zero.wo == 0).all() and (zero.stats == 0).all()


def test_a_zero_row_is_nonpositive(ctx, model, coefs, batch):
    flat, offsets = batch
    mix = np.ascontiguousarray(MIX[:1]).copy()
    mix[0, 5] = 0.0
    o = Out(int(offsets[-1]), 160, levels=2)
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, mix, 1, o)
    assert rc == _lib.F2_ERR_NONPOSITIVE, ctx.lib.f2_last_error(ctx.handle).decode()


@pytest.mark.parametrize("case", ["K=0", "K=65", "mix NULL", "weight nan", "weight inf", "hop=0", "offsets decreasing", "offsets[0]=1",
                                  "offsets NULL", "wave NULL", "coefs NULL", "cnn NULL", "wave_dtype", "fft_precision", "lpf cutoff",
                                  "mem_space", "mem_space async", "C=0", "C=32", "radius=4", "B<0"])
def test_bad_arguments_leave_the_outputs_alone(ctx, model, coefs, batch, case):
    flat, offsets = batch
    mix, k, hop, want = np.ascontiguousarray(MIX).copy(), K, 160, _lib.F2_ERR_INVALID
    kw = {}
    wave, dtype, co = flat, _lib.WAVE_I16, coefs
    if case == "K=0":
        k = 0
    elif case == "K=65":
        mix, k, want = np.tile(np.eye(C), (65, 1, 1)), 65, _lib.F2_ERR_UNSUPPORTED
    elif case == "mix NULL":
        mix = None
    elif case.startswith("weight "):
        mix[1, 3, 2] = float(case.split()[1])
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
    elif case == "lpf cutoff":
        kw.update(lpf=1, cutoff=-5.0)
    elif case == "mem_space":
        kw["mem_space"] = 7
    elif case == "mem_space async":
        kw["mem_space"] = _lib.MEM_HOST_ASYNC
    elif case == "C=0":
        kw["nchan"] = 0
    elif case == "C=32":
        kw["nchan"] = 32                     # the network was built for 16 channels
    elif case == "radius=4":
        kw["radius"] = 4                     # ... and 11 rows
    else:
        kw["nbatch"] = -1
    o = Out(int(batch[1][-1]), 160, levels=max(k, K) + 1)
    rc = raw_sweep(ctx, model, co, wave, dtype, offsets, hop, mix, k, o, **kw)
    assert rc == want, case
    assert o.untouched(), case
    if case.startswith("weight "):
        assert "[1][3][2]" in ctx.lib.f2_last_error(ctx.handle).decode()


def test_errors_come_in_the_headers_order(ctx, model, coefs, batch):
    """what f2_eval_batch_strided rejects first, then the matrices (K, then C's limit is the network's business, then the weights)"""
    flat, offsets = batch
    bad = np.ascontiguousarray(MIX).copy()
    bad[0, 0, 0] = np.nan
    o = Out(int(offsets[-1]), 160, levels=66, env=False)
    message = lambda: ctx.lib.f2_last_error(ctx.handle).decode()
    want = ("scores", "labels", "wo", "stats")
    assert raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 0, bad, K, o, want=want) == _lib.F2_ERR_INVALID and "hop" in message()
    assert raw_sweep(ctx, model, coefs, flat, 9, offsets, 0, None, 0, o, want=want) == _lib.F2_ERR_INVALID and "hop" not in message()
    assert raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, np.tile(bad[:1], (65, 1, 1)), 65, o, want=want) == \
        _lib.F2_ERR_UNSUPPORTED                                                  # too many levels before a weight is looked at
    assert raw_sweep(ctx, model, coefs, None, _lib.WAVE_I16, offsets, 160, bad, K, o, want=want) == _lib.F2_ERR_INVALID
    assert "not finite" in message()                                              # the matrices before the null wave
    assert o.untouched()


# ---- 4. Python layer ------------------------------------------------------------------------------------------------------------------
def test_evaluate_smear_sweep_writes_a_reproducible_npz(tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    from f2cnn_amd import config
    from f2cnn_amd.scripts.CNN import Evaluating
    monkeypatch.chdir(tmp_path)
    config.write_default(nchannels=C)
    m = F2CNNModel.glorot(7, R, C)
    wave = orc.synth_utterance(77, 5000).astype(np.int16)
    wav = str(tmp_path / "DR1.FAAA0.SA1.WAV")
    wavfile.write(wav, 16000, wave)
    hop = 160
    res = Evaluating.EvaluateSmearSweep([wav], spreads=[2, 0.01], bands=[4, C], hop=hop, model=m)[wav]
    first = dict(np.load(str(tmp_path / "DR1.FAAA0.SA1.smearsweep.npz")))
    assert list(np.load(str(tmp_path / "DR1.FAAA0.SA1.smearsweep.npz")).files) == [
        "spread_erb", "bands", "windows", "rising", "agree", "agreement", "hop", "timepoints", "scores", "labels_0", "labels_1", "labels_2",
        "labels_3", "labels_sharp"]
    n = len(range(0, 5000 - R * STEP, hop))
    assert first["windows"].tolist() == [n] * 5 and int(first["hop"]) == hop and first["scores"].shape == (5, n, 2)
    assert np.array_equal(first["spread_erb"], [2.0, 0.01, np.nan, np.nan], equal_nan=True) and first["bands"].tolist() == [0, 0, 4, C]
    assert np.array_equal(first["agreement"], first["agree"] / first["windows"]) and first["agreement"][4] == 1.0
    for k, key in enumerate(("labels_0", "labels_1", "labels_2", "labels_3", "labels_sharp")):
        assert first[key].shape == (n,) and first["rising"][k] == first[key].sum()
        assert first["agree"][k] == (first[key] == first["labels_sharp"]).sum()
        assert np.array_equal(res[key], first[key])
    for k in (1, 3):                                                              # a spread far below the spacing, and C bands
        assert np.array_equal(first["labels_" + str(k)], first["labels_sharp"])
        assert np.array_equal(bits(first["scores"][k]), bits(first["scores"][4]))
    _, sharp_labels = Evaluating.EvaluateOneWavArray(wave, 16000, model=m, hop=hop, LPF=False)
    assert np.array_equal(first["labels_sharp"], sharp_labels)
    printed = capsys.readouterr().out
    assert "agreement with sharp" in printed and "2ERB" in printed and "4bands" in printed and "smear " in printed
