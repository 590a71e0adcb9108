"""The referee of the training step holds its own float32 CPU chain to the acceptance rule, its restatement of the dropout masks
gives Random123's known answers and the keep rates the header promises. No GPU."""
import numpy as np
import pytest

import train_referee as tr


@pytest.mark.parametrize("drop", tr.DROPS, ids=("nodrop", "drop"))
@pytest.mark.parametrize("case", tr.CASES, ids=lambda c: "{}x{}".format(c[2], c[3]))
def test_float32_cpu_chain_is_within_the_measured_error(case, drop):
    """TOL is four times MEASURED, the largest error of this chain over all cases; the chain stays within CHAIN_BOUND = TOL / 2 on
    any machine (train_referee.py says why not MEASURED itself)"""
    ref = tr.referee(*case, drop)
    worst = tr.accept(ref.g32, ref.loss32, ref, "float32 CPU chain {} drop {}".format(case, drop), tol=tr.CHAIN_BOUND)
    assert worst > 0                                   # (the two chains are not the same arithmetic)
    assert tr.errors(ref.g32, ref.loss32, ref)["loss"] <= 2e-7
    assert ref.margin.min() > tr.MARGIN and len(ref.x) == case[4]
    assert set(np.unique(ref.y)) == {0, 1}


def test_restatement_gives_the_published_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = " ".join("{:08x}".format(int(w)) for w in tr.philox4x32_10(counter, key))
        assert got == want, (counter, key)


@pytest.mark.parametrize("rate", (0.25, 0.5, 0.1))
def test_masks_keep_the_promised_fraction(rate):
    per, n = 4 * 63 * 32, 40
    for layer in range(3):
        m = tr.dropout_mask(tr.MASK_SEED, tr.MASK_STEP, layer, np.arange(n), per, rate)
        assert set(np.unique(m)) == {np.float32(0), tr.keep_scale(rate)}
        kept, total = int((m > 0).sum()), n * per
        assert abs(kept - total * (1 - rate)) <= 4 * np.sqrt(total * rate * (1 - rate))
    # the mask depends on the place in the batch, the layer and the step; rate 0 draws nothing
    a = tr.dropout_mask(5, 1, 0, [0, 1], 516, 0.5)
    assert not np.array_equal(a[0], a[1])
    assert not np.array_equal(a, tr.dropout_mask(5, 2, 0, [0, 1], 516, 0.5))
    assert not np.array_equal(a, tr.dropout_mask(5, 1, 1, [0, 1], 516, 0.5))
    assert not np.array_equal(a, tr.dropout_mask(6, 1, 0, [0, 1], 516, 0.5))
    np.testing.assert_array_equal(a, tr.dropout_mask(5, 1, 0, [0, 1], 516, 0.5))
    assert (tr.dropout_mask(5, 1, 0, [0, 1], 516, 0.0) == 1).all()
    # element e uses word e & 3 of the call for e >> 2
    w = tr.philox4x32_10((1, 7, 2, 9), (5, 0))
    m = tr.dropout_mask(5, 9, 2, [7], 8, 0.5)[0]
    np.testing.assert_array_equal(m[4:] > 0, np.array([int(x) for x in w]) * 2.0 ** -32 >= 0.5)
