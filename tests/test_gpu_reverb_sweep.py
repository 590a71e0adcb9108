"""f2_eval_reverb_sweep: a ragged batch at K impulse responses and dry in one device pass. The wet waveforms are held on raw bits
against f2_reverb_levels, the evaluation against f2_eval_batch_strided(F2_WAVE_F64) on the waveforms the call returns, the
device's tally against counts made from the returned labels; the unit response must reproduce the dry level. The batch, the
network and the window geometry of tests/test_gpu_noise_sweep.py, through the C ABI via ctypes."""
import numpy as np
import pytest

import f2cnn_oracle as orc
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.reverb import SyntheticRIR
from test_gpu_noise_sweep import C, LENGTHS, RADIUS, STEP, bits, filled, ragged_waves, tiled_offsets

pytestmark = pytest.mark.gpu

B = len(LENGTHS)                         # (1761, 4000, 1700, 0): one window, a few thousand, none, empty
RIRS = (np.array([1.0]), SyntheticRIR(1.0, 257, seed=1, level=1), SyntheticRIR(1.0, 2000, seed=1, level=2))
K = len(RIRS)
U = (K + 1) * B
FILL = 0x5A
HOPS = (160, 7)


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


@pytest.fixture(scope="module")
def batch():
    return ragged_waves(LENGTHS)


def packed(rirs=RIRS):
    ro = np.zeros(len(rirs) + 1, np.int64)
    ro[1:] = np.cumsum([len(h) for h in rirs])
    return np.concatenate(rirs).astype(np.float64), ro


def n_windows(hop, levels=K + 1, lengths=LENGTHS):
    return levels * sum(_lib.strided_window_count(n, RADIUS, STEP, hop) for n in lengths)


class Out:
    """every output of one call, pre-filled with 0x5A"""

    def __init__(self, total, hop, levels=K + 1, nbatch=B, lengths=LENGTHS):
        self.wet = filled(levels * total, np.float64)
        self.scores = filled((n_windows(hop, levels, lengths), 2), np.float32)
        self.labels = filled(n_windows(hop, levels, lengths), np.uint8)
        self.wo = filled(levels * nbatch + 1, np.int64)
        self.stats = filled((levels * nbatch, 2), np.int64)

    def arrays(self):
        return self.wet, self.scores, self.labels, self.wo, self.stats

    def untouched(self):
        return all((bits(a) == FILL).all() for a in self.arrays())


def raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, rir, ro, k, o, lpf=False, want=("wet", "scores", "labels", "wo", "stats"),
              nbatch=B, mem_space=_lib.MEM_HOST, nchan=C):
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
    g = lambda name: p(getattr(o, name)) if name in want else None
    return ctx.lib.f2_eval_reverb_sweep(ctx.handle, model.handle(ctx), p(wave), dtype, p(offsets), p(coefs), nbatch, nchan, int(lpf),
                                        50.0 if lpf else 0.0, _lib.FFT_F32, RADIUS, STEP, hop, p(rir), p(ro), k, g("wet"),
                                        g("scores"), g("labels"), g("wo"), g("stats"), mem_space)


def sweep(ctx, model, coefs, wave, dtype, offsets, hop, **kw):
    o = Out(int(offsets[-1]), hop)
    rir, ro = packed()
    rc = raw_sweep(ctx, model, coefs, wave, dtype, offsets, hop, rir, ro, K, o, **kw)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    return o


@pytest.fixture(scope="module")
def sweeps(ctx, model, coefs, batch):
    """the int16 batch at both hops: computed once, only read"""
    flat, offsets = batch
    out = {hop: sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop) for hop in HOPS}
    for o in out.values():
        for a in o.arrays():
            a.setflags(write=False)
    return out


def numpy_stats(labels, wo):
    want = np.zeros((U, 2), np.int64)
    for u in range(U):
        mine = labels[wo[u]:wo[u + 1]]
        dry = labels[wo[K * B + u % B]:wo[K * B + u % B + 1]]
        want[u] = mine.sum(), (mine == dry).sum()
    return want


def test_wet_is_reverb_levels(ctx, batch, sweeps):
    flat, offsets = batch
    levels = filled((K + 1) * len(flat), np.float64)
    ctx.reverb_levels(flat, _lib.WAVE_I16, offsets, B, RIRS, levels, _lib.MEM_HOST)
    for hop in HOPS:
        assert np.array_equal(bits(sweeps[hop].wet), bits(levels)), hop
    total = len(flat)
    assert np.array_equal(bits(levels[K * total:]), bits(flat.astype(np.float64)))            # the dry level
    assert np.array_equal(bits(levels[:total]), bits(flat.astype(np.float64)))                # the unit response
    assert not np.array_equal(levels[total:2 * total], levels[:total])


@pytest.mark.parametrize("hop", HOPS)
def test_evaluation_is_the_strided_call_on_the_returned_waveforms(ctx, model, coefs, batch, sweeps, hop):
    _, offsets = batch
    o = sweeps[hop]
    sc, lb = filled((n_windows(hop), 2), np.float32), filled(n_windows(hop), np.uint8)
    wo = ctx.eval_batch_strided(model.handle(ctx), o.wet, _lib.WAVE_F64, tiled_offsets(offsets, K + 1), coefs, U, C, False, 0.0,
                                _lib.FFT_F32, RADIUS, STEP, hop, sc, lb, _lib.MEM_HOST)
    assert np.array_equal(o.wo, wo) and o.wo[-1] == n_windows(hop) > 0
    assert np.array_equal(bits(o.scores), bits(sc))
    assert np.array_equal(o.labels, lb) and set(np.unique(o.labels)) <= {0, 1}


@pytest.mark.parametrize("hop", HOPS)
def test_tally_and_the_unit_response(ctx, model, coefs, batch, sweeps, hop):
    flat, offsets = batch
    o = sweeps[hop]
    want = numpy_stats(o.labels, o.wo)
    print("stats", o.stats.tolist())
    assert np.array_equal(o.stats, want)
    windows = np.diff(o.wo)
    assert np.array_equal(o.stats[K * B:, 1], windows[K * B:])                    # the dry level agrees with itself
    assert (o.stats[windows == 0] == 0).all() and (windows == 0).sum() == 2 * (K + 1)
    # the [1.0] level is the dry level: the same scores on raw bits, full agreement
    nw = int(o.wo[B])
    assert np.array_equal(bits(o.scores[:nw]), bits(o.scores[o.wo[K * B]:]))
    assert np.array_equal(o.stats[:B, 1], windows[:B])
    # every optional output may be NULL; the tally still counts
    quiet = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, want=("stats",))
    assert np.array_equal(quiet.stats, want)
    assert all((bits(a) == FILL).all() for a in (quiet.wet, quiet.scores, quiet.labels, quiet.wo))
    none = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, want=())
    assert none.untouched()


def test_tally_with_both_labels_present(ctx, coefs, batch):
    """The glorot network labels every window of this batch rising. With dense2's bias moved by the median logit difference of
    the dry windows about half of them fall on either side and the rooms move some across."""
    flat, offsets = batch
    hop = 7
    w = dict(orc.glorot_weights(7))
    base = sweep(ctx, F2CNNModel(w), coefs, flat, _lib.WAVE_I16, offsets, hop)
    dry = base.scores[base.wo[K * B]:].astype(np.float64)
    w["dense2_b"] = np.array([np.median(np.log(dry[:, 1]) - np.log(dry[:, 0])), 0.0], np.float32)
    o = sweep(ctx, F2CNNModel(w), coefs, flat, _lib.WAVE_I16, offsets, hop)
    windows = np.diff(o.wo)
    print("windows", windows.tolist(), "stats", o.stats.tolist())
    assert 0 < o.stats[K * B + 1, 0] < windows[K * B + 1]                         # the dry 4000-sample row holds both labels
    assert np.array_equal(o.stats, numpy_stats(o.labels, o.wo))
    assert np.array_equal(o.stats[K * B:, 1], windows[K * B:]) and (o.stats[:, 1] <= windows).all()
    assert np.array_equal(o.stats[:B, 1], windows[:B])                            # the unit response
    assert (o.stats[B:K * B, 1] < windows[B:K * B]).any()                         # some wet window changed sides


def test_float64_waves_and_device_memory_give_the_same_bits(ctx, model, coefs, batch, sweeps):
    flat, offsets = batch
    hop = 160
    ref = sweeps[hop]
    o = sweep(ctx, model, coefs, flat.astype(np.float64), _lib.WAVE_F64, offsets, hop)
    for a, b in zip(o.arrays(), ref.arrays()):
        assert np.array_equal(bits(a), bits(b))
    o = Out(int(offsets[-1]), hop)
    rir, ro = packed()
    dev = [ctx.malloc(max(a.nbytes, 8)) for a in (flat, o.wet, o.scores, o.labels)]
    try:
        for p, a in zip(dev, (flat, o.wet, o.scores, o.labels)):
            ctx.h2d(p, a)
        rc = ctx.lib.f2_eval_reverb_sweep(ctx.handle, model.handle(ctx), dev[0], _lib.WAVE_I16, offsets.ctypes.data, coefs.ctypes.data, B,
                                          C, 0, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, rir.ctypes.data, ro.ctypes.data, K, dev[1], dev[2],
                                          dev[3], o.wo.ctypes.data, o.stats.ctypes.data, _lib.MEM_DEVICE)
        assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
        for p, a in zip(dev[1:], (o.wet, o.scores, o.labels)):
            ctx.d2h(a, p)
    finally:
        ctx.synchronize()
        for p in dev:
            ctx.free(p)
    for a, b in zip(o.arrays(), ref.arrays()):
        assert np.array_equal(bits(a), bits(b))


def test_the_low_pass_goes_down_to_the_strided_call(ctx, model, coefs, batch):
    flat, offsets = batch
    hop = 160
    o = sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, lpf=True)
    sc, lb = filled((n_windows(hop), 2), np.float32), filled(n_windows(hop), np.uint8)
    ctx.eval_batch_strided(model.handle(ctx), o.wet, _lib.WAVE_F64, tiled_offsets(offsets, K + 1), coefs, U, C, True, 50.0, _lib.FFT_F32,
                           RADIUS, STEP, hop, sc, lb, _lib.MEM_HOST)
    assert np.array_equal(bits(o.scores), bits(sc)) and np.array_equal(o.labels, lb)


@pytest.mark.parametrize("case", ["K=0", "K=65", "rir NULL", "rir_offsets NULL", "rir_offsets[0]=1", "rir_offsets decreasing", "no taps",
                                  "tap nan", "32769 taps", "hop=0", "offsets decreasing", "C mismatch", "wave NULL"])
def test_bad_arguments_leave_the_outputs_alone(ctx, model, coefs, batch, case):
    flat, offsets = batch
    (rir, ro), k, hop, nchan, want = packed(), K, 160, C, _lib.F2_ERR_INVALID
    if case == "K=0":
        k = 0
    elif case == "K=65":
        rir, ro, k, want = np.ones(65), np.arange(66, dtype=np.int64), 65, _lib.F2_ERR_UNSUPPORTED
    elif case == "rir NULL":
        rir = None
    elif case == "rir_offsets NULL":
        ro = None
    elif case == "rir_offsets[0]=1":
        ro = ro.copy()
        ro[0] = 1
    elif case == "rir_offsets decreasing":
        ro = ro.copy()
        ro[2] = ro[1] - 1
    elif case == "no taps":
        ro = ro.copy()
        ro[1] = 0
    elif case == "tap nan":
        rir = rir.copy()
        rir[100] = np.nan
    elif case == "32769 taps":
        rir, ro, k, want = np.full(32769, 1e-3), np.array([0, 32769], np.int64), 1, _lib.F2_ERR_UNSUPPORTED
    elif case == "hop=0":
        hop = 0
    elif case == "offsets decreasing":
        offsets = offsets.copy()
        offsets[2] = offsets[1] - 1
    elif case == "C mismatch":
        nchan = C - 1
    else:
        flat = None
    o = Out(int(batch[1][-1]), 160)
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, hop, rir, ro, k, o, nchan=nchan)
    assert rc == want, case
    assert o.untouched(), case


def test_no_window_anywhere_and_the_empty_batch(ctx, model, coefs):
    flat, offsets = ragged_waves((1700, 0), seed=50)
    rir, ro = packed()
    o = Out(1700, 160, nbatch=2, lengths=(1700, 0))
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, offsets, 160, rir, ro, K, o, nbatch=2)
    assert rc == _lib.F2_OK, ctx.lib.f2_last_error(ctx.handle).decode()
    assert (o.wo == 0).all() and (o.stats == 0).all()
    assert np.array_equal(bits(o.wet[K * 1700:]), bits(flat.astype(np.float64)))               # the levels are still made
    empty = Out(0, 160, nbatch=0, lengths=())
    rc = raw_sweep(ctx, model, coefs, flat, _lib.WAVE_I16, np.zeros(1, np.int64), 160, rir, ro, K, empty, nbatch=0)
    assert rc == _lib.F2_OK and empty.wo[0] == 0
