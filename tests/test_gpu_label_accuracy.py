"""f2_label_accuracy: the labels of a strided evaluation against the VTR-derived labels, counted on the device. Every count is
an integer held with == against the referee of tests/label_referee.py, the rule of include/f2cnn_hip.h restated as it reads
(its hand-worked cases are checked first, here and in tests/test_label_accuracy_cli.py).

At hop = STEP nothing is counted in the end-to-end tests, by the rule: ExtractLabel's timepoints are radius*STEP + i*STEP, the
rows of a frame-rate evaluation stand on the same grid in both modes (reference: j*STEP, centre: radius*STEP + j*STEP), and a row
on a timepoint - or a whole step from both neighbours where a label was dropped - is never counted; accuracy is NaN. The same
tests therefore also run at hop 7, where rows fall between the timepoints and every cell of the confusion matrix is in play."""
import os

import numpy as np
import pytest

import f2cnn_oracle as orc
import label_referee as lr
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

STEP = lr.STEP
SENTINEL = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def ctx():
    lr.check_hand_cases()            # the referee first
    c = _lib.Context(0)
    yield c
    c.close()


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


# ---- 1. the hand-worked cases through the library -------------------------------------------------------------------------------
@pytest.mark.parametrize("value", (0, 1))
def test_hand_worked_cases(ctx, value):
    """one utterance of one row per case (origin = t), scored against the case's two labels: with every label `value` the only
    cell that can be 1 is [reference sign][value]"""
    for T, s, t, want in lr.HAND_CASES:
        got = ctx.label_accuracy(np.array([value], np.uint8), [0, 1], [0, 2], T, s, t, 1, STEP, _lib.MEM_HOST)
        expect = np.zeros((1, 2, 2), np.int64)
        if want is not None:
            expect[0, want, value] = 1
        print(T, s, t, want, got.reshape(-1).tolist())
        assert got.dtype == np.int64 and np.array_equal(got, expect), (T, s, t)
    # the cases of a set as rows of one utterance: t = 50 + j
    T, s = [100, 300], [1, 0]
    got = ctx.label_accuracy(np.full(300, value, np.uint8), [0, 300], [0, 2], T, s, 50, 1, STEP, _lib.MEM_HOST)[0]
    expect = np.zeros((2, 2), np.int64)
    expect[1, value], expect[0, value] = 100, 99          # t = 101 .. 200 to the earlier label (the tie with it), 201 .. 299
    assert np.array_equal(got, expect)
    assert np.array_equal(got, lr.referee(np.full(300, value), T, s, 50, 1))


# ---- 2. a ragged random batch against the referee -------------------------------------------------------------------------------
_referee_cache = {}


def ragged_expected(hop, origin):
    """the batch of a case and the referee's (U, 2, 2), computed once per case and not changed afterwards"""
    if (hop, origin) not in _referee_cache:
        batch = lr.ragged_batch(hop, origin)
        conf = lr.ragged_referee(batch, hop, origin)
        assert lr.ragged_condition(conf), "the seed of this case no longer gives counted rows under both signs"
        want = np.stack([conf[u] for u in range(len(lr.ROWS))])
        want.setflags(write=False)
        _referee_cache[(hop, origin)] = (batch, want)
    return _referee_cache[(hop, origin)]


@pytest.mark.parametrize("hop,origin", lr.CASES)
def test_ragged_batch_is_the_referees(ctx, hop, origin):
    (labels, wo, ro, T, s), want = ragged_expected(hop, origin)
    gaps = np.concatenate([np.diff(T[ro[r]:ro[r + 1]]) for r in range(len(lr.SET_SIZES))])
    assert set(lr.GAPS) == set(gaps.tolist())              # every gap width occurs
    host = ctx.label_accuracy(labels, wo, ro, T, s, origin, hop, STEP, _lib.MEM_HOST)
    print("hop", hop, "origin", origin, "counts", host.reshape(len(lr.ROWS), 4).tolist())
    assert np.array_equal(host, want)
    assert (host[:2] == 0).all()                           # no row; a set of one label
    again = ctx.label_accuracy(labels, wo, ro, T, s, origin, hop, STEP, _lib.MEM_HOST)
    assert np.array_equal(again, host)
    d_labels = ctx.malloc(labels.nbytes)
    try:
        ctx.h2d(d_labels, labels)
        dev = ctx.label_accuracy(d_labels, wo, ro, T, s, origin, hop, STEP, _lib.MEM_DEVICE)
        dev2 = ctx.label_accuracy(d_labels, wo, ro, T, s, origin, hop, STEP, _lib.MEM_DEVICE)
    finally:
        ctx.synchronize()
        ctx.free(d_labels)
    assert np.array_equal(dev, want) and np.array_equal(dev2, want)


# ---- 3. the sweep's tiling -------------------------------------------------------------------------------------------------------
def test_utterance_u_is_scored_against_set_u_mod_r(ctx):
    rng = np.random.default_rng(12)
    rows = [300, 0, 77, 1000] * 3
    sizes = [5, 0, 30, 100]
    wo, ro = offsets_of(rows), offsets_of(sizes)
    labels = rng.integers(0, 2, int(wo[-1])).astype(np.uint8)
    T = np.concatenate([np.cumsum(rng.choice(lr.GAPS, n)) for n in sizes]).astype(np.int64)
    s = rng.integers(0, 2, int(ro[-1])).astype(np.uint8)
    hop, origin = 7, 0
    got = ctx.label_accuracy(labels, wo, ro, T, s, origin, hop, STEP, _lib.MEM_HOST)
    assert got.shape == (12, 2, 2)
    for u in range(12):
        r = u % 4
        want = lr.referee(labels[wo[u]:wo[u + 1]], T[ro[r]:ro[r + 1]], s[ro[r]:ro[r + 1]], origin, hop)
        assert np.array_equal(got[u], want), u
    assert got[0].sum() > 0 and got[2].sum() > 0 and got[3].sum() > 0
    assert not np.array_equal(got[0], got[4])              # the same set, other labels


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------
def raw(ctx, labels, wo, U, ro, T, s, R, origin, hop, step, counts, mem_space=_lib.MEM_HOST, handle=True):
    p = lambda a: None if a is None else a.ctypes.data
    return ctx.lib.f2_label_accuracy(ctx.handle if handle else None, p(labels), p(wo), U, p(ro), p(T), p(s), R, origin, hop, step,
                                     p(counts), mem_space)


GOOD = dict(labels=np.array([1, 0, 1, 1], np.uint8), wo=np.array([0, 1, 4], np.int64), U=2, ro=np.array([0, 2], np.int64),
            T=np.array([100, 300], np.int64), s=np.array([1, 0], np.uint8), R=1, origin=150, hop=1, step=STEP)
BAD = {
    "ctx NULL": dict(handle=False),
    "window_offsets NULL": dict(wo=None),
    "ref_offsets NULL": dict(ro=None),
    "counts NULL": dict(counts=None),
    "labels NULL": dict(labels=None),
    "ref_timepoints NULL": dict(T=None),
    "ref_signs NULL": dict(s=None),
    "U < 0": dict(U=-1),
    "R < 1": dict(R=0),
    "U % R": dict(U=2, R=3, ro=np.array([0, 2, 2, 2], np.int64), wo=np.array([0, 1, 4], np.int64)),
    "hop < 1": dict(hop=0),
    "step < 1": dict(step=0),
    "origin < 0": dict(origin=-1),
    "window_offsets[0]": dict(wo=np.array([1, 1, 4], np.int64)),
    "window_offsets decreasing": dict(wo=np.array([0, 4, 3], np.int64)),
    "ref_offsets[0]": dict(ro=np.array([1, 2], np.int64)),
    "ref_offsets decreasing": dict(R=2, ro=np.array([0, 2, 1], np.int64)),
    "timepoints equal": dict(T=np.array([100, 100], np.int64)),
    "timepoints decreasing": dict(T=np.array([300, 100], np.int64)),
    "sign 2": dict(s=np.array([1, 2], np.uint8)),
    "mem_space async": dict(mem_space=_lib.MEM_HOST_ASYNC),
    "mem_space 7": dict(mem_space=7),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_leave_counts_alone(ctx, case):
    args = dict(GOOD, counts=np.full(8, SENTINEL, np.int64))
    args.update(BAD[case])
    counts = args["counts"] if case != "counts NULL" else np.full(8, SENTINEL, np.int64)
    rc = raw(ctx, **args)
    assert rc == _lib.F2_ERR_INVALID, case
    assert (counts == SENTINEL).all(), case
    if case != "ctx NULL":
        with pytest.raises(_lib.F2Error) as e:
            ctx.check(rc)
        assert e.value.code == _lib.F2_ERR_INVALID and str(e.value)


def test_timepoints_may_repeat_across_sets_and_the_good_call_counts(ctx):
    """the arguments the bad cases start from are good; strictly increasing holds inside a set only"""
    counts = np.full(8, SENTINEL, np.int64)
    assert raw(ctx, **dict(GOOD, counts=counts)) == _lib.F2_OK
    # utterance 0: t = 150, label 1 -> [1][1]; utterance 1: t = 150, 151, 152, labels 0 1 1 -> [1][0], 2 x [1][1]
    assert counts.tolist() == [0, 0, 0, 1, 0, 0, 1, 2]
    two = dict(GOOD, R=2, ro=np.array([0, 2, 4], np.int64), T=np.array([100, 300, 100, 300], np.int64), s=np.array([1, 0, 0, 1], np.uint8))
    assert raw(ctx, **dict(two, counts=counts)) == _lib.F2_OK
    assert counts.tolist() == [0, 0, 0, 1, 1, 2, 0, 0]


def test_nothing_to_count_returns_zeros(ctx):
    none = ctx.label_accuracy(np.zeros(0, np.uint8), [0], [0, 2], [100, 300], [1, 0], 0, 1, STEP, _lib.MEM_HOST)
    assert none.shape == (0, 2, 2)
    counts = np.full(1, SENTINEL, np.int64)                # U == 0 writes nothing, with no reference set either
    assert raw(ctx, None, np.zeros(1, np.int64), 0, np.zeros(1, np.int64), None, None, 0, 0, 1, STEP, counts) == _lib.F2_OK
    assert counts[0] == SENTINEL
    counts = np.full((3, 2, 2), SENTINEL, np.int64)        # utterances without rows
    got = ctx.label_accuracy(None, [0, 0, 0, 0], [0, 2], [100, 300], [1, 0], 0, 1, STEP, _lib.MEM_HOST, counts=counts)
    assert (got == 0).all() and (counts == 0).all()
    got = ctx.label_accuracy(np.ones(50, np.uint8), [0, 50], [0, 0], [], [], 0, 1, STEP, _lib.MEM_HOST)    # rows, no labels
    assert (got == 0).all()


# ---- 5. / 6. end to end ------------------------------------------------------------------------------------------------------------
NPZ_KEYS = {None: ["labels", "scores"], 160: ["hop", "labels", "scores", "timepoints"], 7: ["hop", "labels", "scores", "timepoints"]}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """one synthetic file of 1.2 s with .FB / .PHN, the configuration beside it, and the network"""
    from configparser import ConfigParser
    from f2cnn_amd import config
    from f2cnn_amd.scripts.processing import LabelDataGenerator
    root = tmp_path_factory.mktemp("labelled")
    config.write_default(str(root / "configF2CNN.conf"))
    os.makedirs(root / "TEST")
    wav = lr.write_labelled_file(root / "TEST", lambda n: orc.synth_utterance(21, n))
    cp = ConfigParser()
    cp.read(str(root / "configF2CNN.conf"))
    rows = LabelDataGenerator.ExtractLabel(wav, cp)
    assert rows is not None and len(rows) >= 20 and {row[8] for row in rows} == {0, 1}
    return root, wav, F2CNNModel(orc.glorot_weights(7))


_file_results = {}


def file_result(corpus, monkeypatch, capsys, hop, mode):
    """EvaluateOneWavFile(hop, accuracy=mode) on the corpus file, once per (hop, mode): the returned labels, the .npz and what
    the call printed"""
    from f2cnn_amd.scripts.CNN import Evaluating
    root, wav, model = corpus
    monkeypatch.chdir(root)
    if (hop, mode) not in _file_results:
        capsys.readouterr()
        _, labels = Evaluating.EvaluateOneWavFile(wav, hop=hop, model=model, **({} if mode is None else {"accuracy": mode}))
        _file_results[(hop, mode)] = (labels, dict(np.load(os.path.splitext(wav)[0] + ".F2CNN.npz")), capsys.readouterr().out)
    return _file_results[(hop, mode)]


@pytest.mark.parametrize("hop", (160, 7))
@pytest.mark.parametrize("mode", ("reference", "centre"))
def test_evaluate_one_wav_file_scores_against_the_side_files(corpus, monkeypatch, capsys, hop, mode):
    from f2cnn_amd.scripts.CNN import Evaluating
    root, wav, model = corpus
    labels, npz, printed = file_result(corpus, monkeypatch, capsys, hop, mode)
    T, s = Evaluating.ReferenceLabels(wav)
    want = lr.referee(labels, T, s, 0 if mode == "reference" else 5 * STEP, hop)
    print(hop, mode, "confusion", npz["confusion"].tolist(), "accuracy", float(npz["accuracy"]))
    assert sorted(npz) == sorted(NPZ_KEYS[hop] + ["accuracy", "accuracy_mode", "confusion"])
    assert npz["confusion"].dtype == np.int64 and np.array_equal(npz["confusion"], want)
    assert npz["accuracy"].dtype == np.float64 and str(npz["accuracy_mode"]) == mode
    with np.errstate(invalid="ignore"):
        assert np.array_equal(npz["accuracy"], np.float64(np.trace(want)) / np.float64(want.sum()), equal_nan=True)
    assert np.array_equal(npz["labels"], labels) and len(labels) == _lib.strided_window_count(19200, 5, STEP, hop)
    if hop == 7:
        assert want.sum() > 0 and want[0].sum() > 0 and want[1].sum() > 0      # rows between the timepoints: both signs counted
    else:
        assert want.sum() == 0 and np.isnan(npz["accuracy"])                   # rows on the label grid (module docstring)
    assert printed.count("accuracy against the VTR labels ({})".format(mode)) == 1


@pytest.mark.parametrize("hop", (160, None))
def test_without_the_keyword_the_npz_is_todays(corpus, monkeypatch, capsys, hop):
    _, npz, printed = file_result(corpus, monkeypatch, capsys, hop, None)
    assert sorted(npz) == NPZ_KEYS[hop]
    assert "VTR labels" not in printed and "no accuracy" not in printed


def test_a_file_without_side_files_gets_no_accuracy_keys(corpus, monkeypatch, capsys):
    from f2cnn_amd import wavio
    from f2cnn_amd.scripts.CNN import Evaluating
    root, _, model = corpus
    monkeypatch.chdir(root)
    wav = str(root / "TEST" / "DR1.NOFB0.SA2.WAV")
    wavio.write_sphere(wav, 16000, orc.synth_utterance(3, 4000))
    Evaluating.EvaluateOneWavFile(wav, hop=160, model=model, accuracy="centre")
    assert sorted(np.load(os.path.splitext(wav)[0] + ".F2CNN.npz")) == NPZ_KEYS[160]
    assert "no accuracy" in capsys.readouterr().out


@pytest.mark.parametrize("hop", (160, 7))
def test_noise_sweep_scores_every_level(corpus, monkeypatch, capsys, hop):
    from f2cnn_amd.scripts.CNN import Evaluating
    root, wav, model = corpus
    _, clean_npz, _ = file_result(corpus, monkeypatch, capsys, hop, "centre")
    capsys.readouterr()
    res = Evaluating.EvaluateNoiseSweep([wav], [10, 0], hop=hop, model=model, accuracy="centre")[wav]
    printed = capsys.readouterr().out
    saved = dict(np.load(os.path.join("OutputWavFiles", "addedNoise", "DR1.FSYN0.SA1.sweep.npz")))
    T, s = Evaluating.ReferenceLabels(wav)
    assert res["confusion"].shape == (3, 2, 2) and res["confusion"].dtype == np.int64 and res["accuracy_vtr"].shape == (3,)
    for l, key in enumerate(("labels_0", "labels_1", "labels_clean")):
        want = lr.referee(res[key], T, s, 5 * STEP, hop)
        assert np.array_equal(res["confusion"][l], want), key
        with np.errstate(invalid="ignore"):
            assert np.array_equal(res["accuracy_vtr"][l], np.float64(np.trace(want)) / np.float64(want.sum()), equal_nan=True)
    assert np.array_equal(res["confusion"][-1], clean_npz["confusion"])
    assert np.array_equal(saved["confusion"], res["confusion"])
    assert np.array_equal(saved["accuracy_vtr"], res["accuracy_vtr"], equal_nan=True)
    assert printed.count("accuracy against the VTR labels (centre)") == 3
    plain = Evaluating.EvaluateNoiseSweep([wav], [10, 0], hop=hop, model=model)[wav]
    assert "confusion" not in plain and "accuracy_vtr" not in plain
    assert sorted(plain) == sorted(set(res) - {"confusion", "accuracy_vtr"})
