"""The referee of f2_cnn_layers (tests/cnn_layers_referee.py) on the CPU: the float32 PyTorch chain stays at a quarter of TOL32
against the float64 chain on exactly the shapes and inputs the GPU tests use, the float64 chain is the oracle's referee, the
flatten order is dense1's, and the per-element check sees what the scores hide (no GPU needed)."""
import numpy as np
import pytest

import cnn_layers_referee as lr
import f2cnn_oracle as orc

IDS = ["{}x{}x{}-{}".format(*c, k) for c, k in lr.ALL]


@pytest.fixture(scope="module")
def worst():
    return {}


@pytest.mark.parametrize("case,kind", lr.ALL, ids=IDS)
def test_float32_cpu_chain_stays_at_a_quarter_of_the_tolerance(case, kind, worst):
    ref = lr.referee(*case, kind)
    d = lr.dims(case[0], case[1])
    assert ref.pooled64.shape == (case[2], d.flat) and ref.dense64.shape == (case[2], 516) and ref.scores64.shape == (case[2], 2)
    assert np.abs(ref.pooled64).max(axis=1).min() > 0 and np.abs(ref.dense64).max(axis=1).min() > 0    # every window has a scale to compare against
    for layer, a32, a64 in (("pooled", ref.pooled32, ref.pooled64), ("dense1", ref.dense32, ref.dense64)):
        e = float(lr.window_errors(a32, a64).max())
        worst[(case, kind, layer)] = e
        print("float32 CPU chain {} {} {}: worst e_w {:.3g}".format(case, kind, layer, e))
        assert e <= lr.TOL32 / 4, (layer, e)
    assert np.abs(ref.scores32 - ref.scores64).max() <= 2e-5 / 4
    if len(worst) == 2 * len(lr.ALL):
        print("largest e_w of the float32 CPU chain over all cases: {:.3g} (TOL32 = 4 x this = {:.3g})".format(
            max(worst.values()), 4 * max(worst.values())))


@pytest.mark.parametrize("case,kind", lr.ALL, ids=IDS)
def test_float64_chain_is_the_oracles_referee_and_flattens_as_dense1_reads(case, kind):
    ref = lr.referee(*case, kind)
    truth = orc.cnn_forward_referee(ref.x, dict(ref.model.tensors))
    assert np.abs(ref.scores64 - truth).max() <= 1e-12
    # (h, w, c): the pooled array through dense1_w as the model holds it, in numpy float64, is the chain's own dense1
    again = lr.dense1_of(ref.pooled64, ref.model)
    assert np.abs(again - ref.dense64).max() <= 1e-12 * np.abs(ref.dense64).max()
    d = lr.dims(case[0], case[1])
    if d.Hp2 * d.Wp2 > 1:      # ... and no other order is: channel-major (NCHW) flattening gives another dense1
        nchw = ref.pooled64.reshape(-1, d.Hp2, d.Wp2, 64).transpose(0, 3, 1, 2).reshape(len(ref.x), -1)
        assert np.abs(lr.dense1_of(nchw, ref.model) - ref.dense64).max() > 1e-3 * np.abs(ref.dense64).max()


def scores_of(dense1, model):
    z = dense1 @ model.tensors["dense2_w"].astype(np.float64) + model.tensors["dense2_b"].astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("case", [(11, 128, 193), (13, 40, 33), (18, 20, 33)], ids=lambda c: "{}x{}".format(c[0], c[1]))
def test_the_check_sees_a_lost_lo_piece_in_one_column_and_the_scores_do_not(case):
    """The gap this referee closes: the last pooled column off by 2^-11 relative (a whole fp16 `lo` piece lost in one edge tile)
    fails the per-element check at the split routes' tolerance, while the scores move by less than the 2e-5 they are held to."""
    ref = lr.referee(*case, "unit")
    d = lr.dims(case[0], case[1])
    bad = ref.pooled64.reshape(-1, d.Hp2, d.Wp2, 64).copy()
    bad[:, :, -1, :] *= 1.0 + 2.0 ** -11
    bad = bad.reshape(len(ref.x), -1)
    with pytest.raises(AssertionError, match="pooled column {}".format(d.Wp2 - 1)):
        lr.check("pooled", bad, ref.pooled64, lr.TOL_SPLIT, case[0], case[1])
    moved = np.abs(scores_of(lr.dense1_of(bad, ref.model), ref.model) - ref.scores64).max()
    print("{}: last pooled column x (1 + 2^-11) moves the scores by {:.3g}".format(case, moved))
    assert moved < 2e-5
    lr.check("pooled", ref.pooled64.astype(np.float32), ref.pooled64, lr.TOL32, case[0], case[1])     # float32 rounding alone passes
    # a dense1 unit off by as much is seen too, and named
    unit = int(np.argmax(ref.dense64[0]))
    bad1 = ref.dense64.copy()
    bad1[:, unit] *= 1.0 + 2.0 ** -11
    with pytest.raises(AssertionError, match="dense unit {}:".format(unit)):
        lr.check("dense1", bad1, ref.dense64, lr.TOL_SPLIT, case[0], case[1])
