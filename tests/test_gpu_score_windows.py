"""f2_cnn_score_windows (`cnn test`): stored raw windows normalised on the device, scored by the forward chain and tallied by
sign, label and group. References: normalizeInputBatch (K3) + f2_cnn_forward for the scores and labels, bit for bit; NumPy for
the counts; math.fsum of the float64 terms for the loss."""
import csv
import json
import math

import numpy as np
import pytest

from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.scripts.CNN import Training

pytestmark = pytest.mark.gpu

ROWS = 11
N_BIG = 16384 + 3          # crosses the boundary of the 16384-window chunks
SENTINEL_I, SENTINEL_D = -12345, -6.5


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def raw_windows(seed, n, channels):
    """strictly positive raw windows; none is constant (checked here, on the CPU)"""
    w = np.exp(np.random.default_rng(seed).normal(0.0, 1.0, (n, ROWS, channels))).astype(np.float32)
    flat = w.reshape(n, -1)
    assert (flat > 0).all() and (flat.min(axis=1) < flat.max(axis=1)).all()
    return w


def forward(ctx, model, x):
    x = np.ascontiguousarray(x, np.float32)
    scores, labels = np.empty((len(x), 2), np.float32), np.empty(len(x), np.uint8)
    ctx.cnn_forward(model.handle(ctx), x, len(x), scores, labels, _lib.MEM_HOST)
    return scores, labels


def forward_device(ctx, model, x):
    x = np.ascontiguousarray(x, np.float32)
    n = len(x)
    scores, labels = np.empty((n, 2), np.float32), np.empty(n, np.uint8)
    d_x, d_s, d_l = ctx.malloc(x.nbytes), ctx.malloc(scores.nbytes), ctx.malloc(n)
    try:
        ctx.h2d(d_x, x)
        ctx.cnn_forward(model.handle(ctx), d_x, n, d_s, d_l, _lib.MEM_DEVICE)
        ctx.synchronize()
        ctx.d2h(scores, d_s)
        ctx.d2h(labels, d_l)
    finally:
        for p in (d_x, d_s, d_l):
            ctx.free(p)
    return scores, labels


def score(ctx, model, w, signs, groups=None, G=1, normalize=True, mem=_lib.MEM_HOST, want=True):
    """(scores, labels, counts, loss_sum) of one call; with mem = MEM_DEVICE everything the header puts in mem_space lives there"""
    w = np.ascontiguousarray(w, np.float32)
    n = len(w)
    signs = np.ascontiguousarray(signs, np.uint8)
    groups = None if groups is None else np.ascontiguousarray(groups, np.int32)
    scores, labels = (np.empty((n, 2), np.float32), np.empty(n, np.uint8)) if want else (None, None)
    if mem == _lib.MEM_HOST:
        counts, loss = ctx.cnn_score_windows(model.handle(ctx), w, n, normalize, signs, groups, G, scores, labels, mem)
        return scores, labels, counts, loss
    held = []

    def up(a):
        p = ctx.malloc(max(a.nbytes, 4))
        held.append(p)
        ctx.h2d(p, a)
        return p
    try:
        d_w, d_signs = up(w), up(signs)
        d_groups = None if groups is None else up(groups)
        d_s, d_l = (up(scores), up(labels)) if want else (None, None)
        counts, loss = ctx.cnn_score_windows(model.handle(ctx), d_w, n, normalize, d_signs, d_groups, G, d_s, d_l, mem)
        if want:
            ctx.d2h(scores, d_s)
            ctx.d2h(labels, d_l)
    finally:
        for p in held:
            ctx.free(p)
    return scores, labels, counts, loss


def numpy_counts(labels, signs, groups, G):
    out = np.zeros((G, 2, 2), np.int64)
    np.add.at(out, (np.zeros(len(labels), np.int64) if groups is None else groups, signs, (labels != 0).astype(np.int64)), 1)
    return out


def fsum_loss(scores, signs, groups, G):
    p = np.clip(scores[np.arange(len(signs)), signs].astype(np.float64), 1e-7, 1.0)
    terms = -np.log(p)
    g = np.zeros(len(signs), np.int64) if groups is None else groups
    return [math.fsum(terms[g == k].tolist()) for k in range(G)]


def assert_loss(loss, scores, signs, groups, G):
    ref = fsum_loss(scores, signs, groups, G)
    n_g = np.bincount(np.zeros(len(signs), np.int64) if groups is None else groups, minlength=G)
    for k in range(G):
        err, bound = abs(loss[k] - ref[k]), (n_g[k] + 8) * 2.0 ** -52 * ref[k]
        assert err <= bound, (k, loss[k], ref[k], err, bound)


# ---- shared inputs and references (computed once, never written to) ---------------------------------------------------------
@pytest.fixture(scope="module")
def model40():
    return F2CNNModel.glorot(seed=7, rows=ROWS, channels=40)


@pytest.fixture(scope="module")
def big40(ctx, model40):
    """N_BIG raw 11 x 40 windows, their K3-normalised form, f2_cnn_forward's scores / labels on it, signs"""
    w = raw_windows(11, N_BIG, 40)
    x = Training.normalizeInputBatch(w, ctx)
    scores, labels = forward(ctx, model40, x)
    signs = np.random.default_rng(5).integers(0, 2, N_BIG).astype(np.uint8)
    for a in (w, x, scores, labels, signs):
        a.flags.writeable = False
    return w, x, scores, labels, signs


@pytest.fixture(scope="module")
def mixed40(ctx, model40, big40):
    """the glorot network with dense2's bias moved by the median logit difference: about half the windows on either side"""
    s = big40[2][:2000].astype(np.float64)
    t = dict(model40.tensors)
    t["dense2_b"] = np.array([np.median(np.log(s[:, 1]) - np.log(s[:, 0])), 0.0], np.float32)
    return F2CNNModel(t, ROWS, 40)


# ---- 1. normalisation parity ------------------------------------------------------------------------------------------------
def adversarial(channels):
    rng = np.random.default_rng(3)
    w = raw_windows(21, 6, channels)
    w[0] = 3.25                                                               # constant: zeros
    w[1] = (10.0 ** rng.uniform(-30, 30, (ROWS, channels))).astype(np.float32)
    w[1, 0, 0], w[1, 0, 1] = 1e-30, 1e30
    w[2, 4, 7] = np.float32(1e-41)                                            # a float32 denormal is the minimum
    w[3] = np.float32(1e-42) * (1 + np.arange(ROWS * channels, dtype=np.float32).reshape(ROWS, channels))   # denormals only
    w[4] = np.nextafter(np.float32(1.0), np.float32(2.0), dtype=np.float32)
    w[4, 10, channels - 1] = 1.0                                              # two neighbouring floats
    assert (w > 0).all() and np.isfinite(w).all() and w[3].max() < np.finfo(np.float32).tiny
    return w


@pytest.mark.parametrize("channels,seed", [(40, 7), (40, 19), (67, 7), (67, 19)])
def test_normalisation_matches_k3_on_adversarial_windows(ctx, channels, seed):
    model = F2CNNModel.glorot(seed=seed, rows=ROWS, channels=channels)
    w = adversarial(channels)
    assert w[0].size == ROWS * channels and (channels != 67 or w[0].size == 737)
    x = Training.normalizeInputBatch(w, ctx)
    assert not x[0].any() and x[1:].max() == 1.0 and x[1:].min() == 0.0
    ref_s, ref_l = forward(ctx, model, x)
    signs = np.zeros(len(w), np.uint8)
    s, l, _, _ = score(ctx, model, w, signs)
    assert np.array_equal(s.view(np.uint32), ref_s.view(np.uint32)) and np.array_equal(l, ref_l)
    zero_s, _ = forward(ctx, model, np.zeros((1, ROWS, channels), np.float32))
    assert np.array_equal(s[0].view(np.uint32), zero_s[0].view(np.uint32))    # the constant window: an all-zero input
    for i in range(len(w)):                                                   # n = 1, every window alone
        s1, l1, _, _ = score(ctx, model, w[i:i + 1], signs[:1])
        assert np.array_equal(s1.view(np.uint32), ref_s[i:i + 1].view(np.uint32)) and l1[0] == ref_l[i], i


# ---- 2. scores and labels are f2_cnn_forward's bits -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, N_BIG])
def test_normalised_scores_and_labels_are_cnn_forward_bits(ctx, model40, big40, n):
    w, x, ref_s, ref_l, signs = big40
    if n < N_BIG:                                                            # (the reference of a sub-batch: the same rows - checked)
        s_n, l_n = forward(ctx, model40, x[:n])
        assert np.array_equal(s_n.view(np.uint32), ref_s[:n].view(np.uint32)) and np.array_equal(l_n, ref_l[:n])
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        s, l, counts, _ = score(ctx, model40, w[:n], signs[:n], mem=mem)
        assert np.array_equal(s.view(np.uint32), ref_s[:n].view(np.uint32)), mem
        assert np.array_equal(l, ref_l[:n]), mem
        assert np.array_equal(counts, numpy_counts(l, signs[:n], None, 1))


@pytest.mark.parametrize("n", [1, 257, N_BIG])
def test_unnormalised_scores_and_labels_are_cnn_forward_bits(ctx, model40, n):
    """normalize = 0 with max |x| = 100 in every chunk: the range pass picks B = 128"""
    x = np.random.default_rng(n).uniform(-100.0, 100.0, (n, ROWS, 40)).astype(np.float32)
    x[:, 0, 0] = 100.0
    signs = np.random.default_rng(6).integers(0, 2, n).astype(np.uint8)
    ref_s, ref_l = forward(ctx, model40, x)
    assert ctx.cnn_info(model40.handle(ctx), "last_input_bound") == 128.0
    dev_s, dev_l = forward_device(ctx, model40, x)
    assert np.array_equal(dev_s.view(np.uint32), ref_s.view(np.uint32)) and np.array_equal(dev_l, ref_l)
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        s, l, counts, loss = score(ctx, model40, x, signs, normalize=False, mem=mem)
        assert np.array_equal(s.view(np.uint32), ref_s.view(np.uint32)), mem
        assert np.array_equal(l, ref_l), mem
        assert np.array_equal(counts, numpy_counts(l, signs, None, 1))
        assert_loss(loss, s, signs, None, 1)


def test_last_input_bound_follows_an_unnormalised_call_only(ctx, model40, big40):
    """normalize = 0 takes f2_cnn_forward's route and leaves its record too; normalize = 1 measures no range and leaves it alone"""
    info = lambda: ctx.cnn_info(model40.handle(ctx), "last_input_bound")
    n = 300
    x = np.random.default_rng(3).uniform(-100.0, 100.0, (n, ROWS, 40)).astype(np.float32)
    x[0, 0, 0] = 100.0
    signs = big40[4][:n]
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        forward(ctx, model40, big40[1][:4])                                  # inputs in [0, 1]
        assert info() == 1.0
        score(ctx, model40, x, signs, normalize=False, mem=mem, want=False)
        assert info() == 128.0, mem
        score(ctx, model40, big40[0][:n], signs, normalize=True, mem=mem, want=False)
        assert info() == 128.0, mem


def test_128_channels_take_the_weight_stationary_kernels(ctx):
    model = F2CNNModel.glorot(seed=7, rows=ROWS, channels=128)
    assert ctx.cnn_info(model.handle(ctx), "ws_ok") == 1.0
    n = 300
    w = raw_windows(31, n, 128)
    signs = np.random.default_rng(8).integers(0, 2, n).astype(np.uint8)
    groups = np.random.default_rng(9).integers(0, 3, n).astype(np.int32)
    x = Training.normalizeInputBatch(w, ctx)
    ref_s, ref_l = forward(ctx, model, x)
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        s, l, counts, loss = score(ctx, model, w, signs, groups, 3, mem=mem)
        assert np.array_equal(s.view(np.uint32), ref_s.view(np.uint32)) and np.array_equal(l, ref_l), mem
        assert np.array_equal(counts, numpy_counts(l, signs, groups, 3))
        assert_loss(loss, s, signs, groups, 3)
    s0, l0, _, _ = score(ctx, model, x, signs, groups, 3, normalize=False)
    assert np.array_equal(s0.view(np.uint32), ref_s.view(np.uint32)) and np.array_equal(l0, ref_l)


# ---- 3. counts --------------------------------------------------------------------------------------------------------------
def group_case(case, n):
    rng = np.random.default_rng(17)
    if case == "G=1 NULL":
        return None, 1
    if case == "G=7 one empty":
        g = rng.integers(0, 6, n).astype(np.int32)
        g[g >= 3] += 1                                                       # group 3 stays empty
        return g, 7
    if case == "G=1024":
        return rng.integers(0, 1024, n).astype(np.int32), 1024
    return np.full(n, 6, np.int32), 7                                        # all in the last group


@pytest.mark.parametrize("case", ["G=1 NULL", "G=7 one empty", "G=1024", "all last"])
@pytest.mark.parametrize("mem", [_lib.MEM_HOST, _lib.MEM_DEVICE])
def test_counts_equal_the_numpy_tally(ctx, mixed40, big40, case, mem):
    n = 2000
    w, signs = big40[0][:n], big40[4][:n]
    groups, G = group_case(case, n)
    s, l, counts, loss = score(ctx, mixed40, w, signs, groups, G, mem=mem)
    rising = int((l != 0).sum())
    print(case, "rising", rising, "of", n)
    assert 0 < rising < n                                                    # the network's labels are mixed
    assert counts.sum() == n
    assert np.array_equal(counts, numpy_counts(l, signs, groups, G))
    if case == "G=7 one empty":
        assert not counts[3].any() and loss[3] == 0.0
    assert_loss(loss, s, signs, groups, G)
    # the tally runs without the caller's scores and labels too
    _, _, counts2, loss2 = score(ctx, mixed40, w, signs, groups, G, mem=mem, want=False)
    assert np.array_equal(counts2, counts) and np.array_equal(loss2.view(np.uint64), loss.view(np.uint64))


# ---- 4. loss ----------------------------------------------------------------------------------------------------------------
def test_loss_across_the_chunk_boundary_repeats_bit_for_bit(ctx, mixed40, big40):
    w, signs = big40[0], big40[4]
    groups = (np.arange(N_BIG) % 5).astype(np.int32)
    s, l, counts, loss = score(ctx, mixed40, w, signs, groups, 5)
    assert np.array_equal(counts, numpy_counts(l, signs, groups, 5))
    assert_loss(loss, s, signs, groups, 5)
    _, _, counts2, loss2 = score(ctx, mixed40, w, signs, groups, 5)
    assert np.array_equal(counts2, counts) and np.array_equal(loss2.view(np.uint64), loss.view(np.uint64))
    _, _, counts3, loss3 = score(ctx, mixed40, w, signs, groups, 5, mem=_lib.MEM_DEVICE)
    assert np.array_equal(counts3, counts) and np.array_equal(loss3.view(np.uint64), loss.view(np.uint64))


def test_loss_clips_scores_of_zero_and_one(ctx, model40, big40):
    """dense2_w x 1000. On the normalised windows this network's logits differ by less than 0.05, so the sharpened scores fall
    below 1e-7 (clipped) without reaching float32's underflow; the same windows x 64, taken as they are, scale the logits of the
    bias-free network by 64 as well: true-class scores of exactly 0 (each contributes -ln 1e-7) and exactly 1 (contributes 0)."""
    n = 2000
    w, x, signs = big40[0][:n], big40[1][:n], big40[4][:n]
    t = dict(model40.tensors)
    assert not any(t[k].any() for k in t if k.endswith("_b"))
    t["dense2_w"] = t["dense2_w"] * np.float32(1000.0)
    sharp = F2CNNModel(t, ROWS, 40)
    groups = (np.arange(n) % 3).astype(np.int32)
    s, _, _, loss = score(ctx, sharp, w, signs, groups, 3)
    true = s[np.arange(n), signs]
    print("normalised: true-class scores below 1e-7:", int((true < 1e-7).sum()), "exactly 0:", int((true == 0.0).sum()))
    assert (true < 1e-7).any()
    assert_loss(loss, s, signs, groups, 3)
    s, _, _, loss = score(ctx, sharp, x * np.float32(64.0), signs, groups, 3, normalize=False)
    true = s[np.arange(n), signs]
    zeros, ones = int((true == 0.0).sum()), int((true == 1.0).sum())
    print("x 64: true-class scores of exactly 0:", zeros, "of exactly 1:", ones, "of", n)
    assert zeros > 0 and ones > 0
    assert_loss(loss, s, signs, groups, 3)
    if zeros + ones == n:                                                    # then the sum is zeros x -ln 1e-7
        assert loss.sum() == pytest.approx(zeros * -math.log(1e-7), rel=1e-13)
    s2, _, _, loss2 = score(ctx, sharp, x * np.float32(64.0), signs, groups, 3, normalize=False)
    assert np.array_equal(loss2.view(np.uint64), loss.view(np.uint64)) and np.array_equal(s2, s)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------
def call(ctx, model, w, signs, groups, G, normalize=1, mem=_lib.MEM_HOST, n=None, counts="own", null_loss=False):
    """the raw entry point; returns (status, counts, loss_sum) with the outputs pre-filled with sentinels"""
    c = np.full((max(G, 1) + 2, 2, 2), SENTINEL_I, np.int64)
    d = np.full(max(G, 1) + 2, SENTINEL_D, np.float64)
    rc = ctx.lib.f2_cnn_score_windows(ctx.handle, model.handle(ctx), _lib._ptr(w), len(w) if n is None else n, normalize,
                                      _lib._ptr(signs), _lib._ptr(groups), G, None, None, None if counts is None else _lib._ptr(c),
                                      None if null_loss else _lib._ptr(d), mem)
    return rc, c, d


@pytest.mark.parametrize("bad", ["zero", "negative", "nan", "all three"])
def test_nonpositive_values_are_reported(ctx, model40, big40, bad):
    w = np.array(big40[0][:300])
    if bad in ("zero", "all three"):
        w[3, 2, 5] = 0.0
    if bad in ("negative", "all three"):
        w[150, 10, 39] = -1.0
    if bad in ("nan", "all three"):
        w[299, 0, 0] = np.nan
    rc, _, _ = call(ctx, model40, w, np.zeros(300, np.uint8), None, 1)
    assert rc == _lib.F2_ERR_NONPOSITIVE
    assert "positive" in ctx.lib.f2_last_error(ctx.handle).decode()
    if bad in ("zero", "negative"):                                          # taken as they are, such windows are no error
        rc, c, _ = call(ctx, model40, w, np.zeros(300, np.uint8), None, 1, normalize=0)
        assert rc == _lib.F2_OK and c[0].sum() == 300


def test_bad_signs_and_groups_are_found_by_the_tally(ctx, model40, big40):
    w = big40[0][:300]
    signs = np.zeros(300, np.uint8)
    groups = (np.arange(300) % 4).astype(np.int32)
    bad_signs = signs.copy()
    bad_signs[277] = 2
    rc, _, _ = call(ctx, model40, w, bad_signs, groups, 4)
    assert rc == _lib.F2_ERR_INVALID and "sign" in ctx.lib.f2_last_error(ctx.handle).decode()
    for value in (4, -1):
        g = groups.copy()
        g[13] = value
        rc, _, _ = call(ctx, model40, w, signs, g, 4)
        assert rc == _lib.F2_ERR_INVALID and "group" in ctx.lib.f2_last_error(ctx.handle).decode(), value
    rc, c, _ = call(ctx, model40, w, signs, groups, 4)                       # and the same call with good data passes
    assert rc == _lib.F2_OK and c[:4].sum() == 300


@pytest.mark.parametrize("case", ["G=0", "G=1025", "NULL groups G=2", "n=-1", "normalize=2", "HOST_ASYNC", "NULL counts",
                                  "NULL loss_sum", "NULL windows", "NULL signs", "NULL cnn"])
def test_bad_arguments_leave_the_outputs_alone(ctx, model40, big40, case):
    w = big40[0][:64]
    signs = np.zeros(64, np.uint8)
    groups = np.zeros(64, np.int32)
    kw = dict(w=w, signs=signs, groups=groups, G=2)
    expect = _lib.F2_ERR_INVALID
    if case == "G=0":
        kw["G"] = 0
    elif case == "G=1025":
        kw["G"], expect = 1025, _lib.F2_ERR_UNSUPPORTED
    elif case == "NULL groups G=2":
        kw["groups"] = None
    elif case == "n=-1":
        kw["n"] = -1
    elif case == "normalize=2":
        kw["normalize"] = 2
    elif case == "HOST_ASYNC":
        kw["mem"] = _lib.MEM_HOST_ASYNC
    elif case == "NULL counts":
        kw["counts"] = None
    elif case == "NULL loss_sum":
        kw["null_loss"] = True
    elif case == "NULL windows":
        kw["w"], kw["n"] = None, 64
    elif case == "NULL signs":
        kw["signs"] = None
    if case == "NULL cnn":
        c = np.full((4, 2, 2), SENTINEL_I, np.int64)
        d = np.full(4, SENTINEL_D, np.float64)
        rc = ctx.lib.f2_cnn_score_windows(ctx.handle, None, _lib._ptr(w), 64, 1, _lib._ptr(signs), _lib._ptr(groups), 2, None, None,
                                          _lib._ptr(c), _lib._ptr(d), _lib.MEM_HOST)
    else:
        rc, c, d = call(ctx, model40, kw.pop("w"), kw.pop("signs"), kw.pop("groups"), kw.pop("G"), **kw)
    assert rc == expect
    assert (c == SENTINEL_I).all() and (d == SENTINEL_D).all()
    assert ctx.lib.f2_last_error(ctx.handle).decode()


def test_null_context_and_no_windows(ctx, model40):
    c = np.full((3, 2, 2), SENTINEL_I, np.int64)
    d = np.full(3, SENTINEL_D, np.float64)
    assert ctx.lib.f2_cnn_score_windows(None, model40.handle(ctx), None, 0, 1, None, None, 1, None, None, _lib._ptr(c), _lib._ptr(d),
                                        _lib.MEM_HOST) == _lib.F2_ERR_INVALID
    assert (c == SENTINEL_I).all()
    rc = ctx.lib.f2_cnn_score_windows(ctx.handle, model40.handle(ctx), None, 0, 1, None, _lib._ptr(np.zeros(1, np.int32)), 3, None,
                                      None, _lib._ptr(c), _lib._ptr(d), _lib.MEM_HOST)
    assert rc == _lib.F2_OK and not c.any() and not d.any()


# ---- 6. Python layer ----------------------------------------------------------------------------------------------------------
def test_model_evaluate_gives_the_training_scripts_lines(ctx, mixed40, big40):
    n = 500
    w, signs = big40[0][:n], big40[4][:n]
    x = Training.normalizeInputBatch(w, ctx)
    y = signs.astype(np.int64)
    scores, labels = mixed40.predict_labels(x, ctx)                          # the last lines of TrainAndPlotLoss
    p = np.clip(scores[np.arange(n), y].astype(np.float64), 1e-7, 1.0)
    want_loss, want_acc = float(-np.log(p).mean()), float((labels == y).mean())
    loss, acc = mixed40.evaluate(w, y, normalize=True, ctx=ctx)
    assert acc == want_acc and 0.0 < acc < 1.0
    assert abs(loss - want_loss) <= (n + 8) * 2.0 ** -52 * want_loss
    loss0, acc0 = mixed40.evaluate(x[..., None], y, ctx=ctx)                 # already normalised, Keras' trailing axis
    assert acc0 == want_acc and loss0 == loss
    groups = np.arange(n) % 3
    lg, ag, counts, loss_sum = mixed40.evaluate(w, y, groups=groups, n_groups=3, normalize=True, ctx=ctx)
    assert ag == want_acc and counts.shape == (3, 2, 2) and counts.sum() == n
    assert np.array_equal(counts, numpy_counts(labels, y, groups, 3))
    assert lg == float(loss_sum.sum()) / n
    with pytest.raises(ValueError):
        mixed40.evaluate(w, np.full(n, 2), ctx=ctx)


def test_testmodel_on_a_small_corpus(ctx, mixed40, big40, tmp_path, capsys, monkeypatch):
    n = 60
    w = np.array(big40[0][:n])
    rng = np.random.default_rng(2)
    phonemes, regions = ("aa", "iy", "w"), ("DR1", "DR5")
    rows = [["TEST" if i % 3 == 0 else "TRAIN", regions[i % 2], "SPK%d" % (i % 7), "SX%d" % i, phonemes[int(rng.integers(0, 3))],
             str(800 + 160 * i), "%.3f" % rng.normal(), "0.01", str(int(rng.integers(0, 2)))] for i in range(n)]
    with open(tmp_path / "label_data.csv", "w", newline="") as f:
        csv.writer(f).writerows(rows)
    np.save(tmp_path / "input_data.npy", w)
    path = str(tmp_path / "last_trained_model")
    mixed40.save(path)
    res = Training.TestModel(labelFile=str(tmp_path / "label_data.csv"), inputFile=str(tmp_path / "input_data.npy"), model=path,
                             by="phoneme", rows="all", ctx=ctx)
    out = capsys.readouterr().out
    assert "Test loss:" in out and "Test accuracy:" in out and all(p in out for p in phonemes)
    assert json.load(open(path + "_test.json")) == res
    signs = np.array([int(r[8]) for r in rows])
    names = sorted({r[4] for r in rows})
    groups = np.array([names.index(r[4]) for r in rows])
    scores, labels = mixed40.predict_labels(Training.normalizeInputBatch(w, ctx), ctx)
    want = numpy_counts(labels, signs, groups, len(names))
    ref_loss = fsum_loss(scores, signs, groups, len(names))
    assert res["windows"] == n and [g["name"] for g in res["groups"]] == names
    assert res["accuracy"] == float((labels == signs).mean())
    for k, g in enumerate(res["groups"]):
        assert g["counts"] == want[k].tolist() and g["windows"] == int(want[k].sum())
        assert g["accuracy"] == float(want[k][0, 0] + want[k][1, 1]) / g["windows"]
        assert abs(g["loss_sum"] - ref_loss[k]) <= (g["windows"] + 8) * 2.0 ** -52 * ref_loss[k]
        assert g["loss"] == g["loss_sum"] / g["windows"]
    assert abs(res["loss"] * n - math.fsum(ref_loss)) <= (n + 8) * 2.0 ** -52 * math.fsum(ref_loss)
    # the TEST rows alone: a third of the corpus
    res_t = Training.TestModel(labelFile=str(tmp_path / "label_data.csv"), inputFile=str(tmp_path / "input_data.npy"), model=path,
                               by="region", rows="test", ctx=ctx)
    assert res_t["windows"] == 20 and [g["name"] for g in res_t["groups"]] == ["DR1", "DR5"]
    sel = np.arange(0, n, 3)
    assert sum(g["counts"][0][0] + g["counts"][1][1] for g in res_t["groups"]) == int((labels[sel] == signs[sel]).sum())
    # a model named with its .npz: the result lies beside it without the suffix; a model object: nothing is written
    mixed40.save(str(tmp_path / "w.npz"))
    res_n = Training.TestModel(labelFile=str(tmp_path / "label_data.csv"), inputFile=str(tmp_path / "input_data.npy"),
                               model=str(tmp_path / "w.npz"), by="region", rows="test", ctx=ctx)
    assert json.load(open(tmp_path / "w_test.json")) == res_n and res_n["groups"] == res_t["groups"]
    monkeypatch.chdir(tmp_path)
    before = sorted(p.name for p in tmp_path.iterdir())
    res_o = Training.TestModel(labelFile="label_data.csv", inputFile="input_data.npy", model=mixed40, by="region", rows="test", ctx=ctx)
    assert res_o["model"] is None and res_o["groups"] == res_t["groups"]
    assert sorted(p.name for p in tmp_path.iterdir()) == before
    assert "Results saved" not in capsys.readouterr().out.split("Test accuracy:")[-1]
