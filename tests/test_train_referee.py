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


def test_float32_cpu_chain_past_the_first_chunk():
    """CHUNK_CASE: 1094 selected windows with dropout, 70 of them at places >= 1024"""
    ref = tr.referee(*tr.CHUNK_CASE, tr.DROP)
    tr.accept(ref.g32, ref.loss32, ref, "float32 CPU chain {} drop {}".format(tr.CHUNK_CASE, tr.DROP), tol=tr.CHAIN_BOUND)
    assert tr.errors(ref.g32, ref.loss32, ref)["loss"] <= 2e-7
    assert ref.margin.min() > tr.MARGIN and len(ref.x) == 1094 and set(np.unique(ref.y)) == {0, 1}
    # the places behind 1024 have masks of their own: a chain that gave them the masks of the places 0 .. 69 is another chain
    m = tr.masks_for(np.arange(1024, 1094), tr.CHUNK_CASE[2], tr.CHUNK_CASE[3], tr.DROP)
    assert all(np.array_equal(a, b[1024:]) and not np.array_equal(a, b[:70]) for a, b in zip(m, ref.masks))


def test_saturated_softmax_case():
    """dense2 times SATURATION_GAIN: the promised shares of saturated and unsaturated windows, the same windows as without the gain,
    and the float32 CPU chain within CHAIN_BOUND"""
    plain = tr.referee(*tr.CASES[0], tr.DROPS[0])
    ref = tr.referee(*tr.CASES[0], tr.DROPS[0], dense2_gain=tr.SATURATION_GAIN)
    assert ref.x.tobytes() == plain.x.tobytes() and ref.y.tobytes() == plain.y.tobytes() and ref.tried == plain.tried
    for k, gain in zip(("dense2_w", "dense2_b"), tr.SATURATION_GAIN):
        np.testing.assert_array_equal(ref.model.tensors[k], plain.model.tensors[k] * np.float32(gain))
    assert all(np.array_equal(ref.model.tensors[k], plain.model.tensors[k]) for k in tr.TENSORS[:10])
    gap = np.abs(ref.z64[:, 1] - ref.z64[:, 0])
    n = len(gap)
    print("|z1 - z0|: min {:.3g} median {:.3g} max {:.3g}; {} of {} above {}, {} below {}; loss {:.6g}".format(
        gap.min(), np.median(gap), gap.max(), int((gap > tr.SATURATED).sum()), n, tr.SATURATED, int((gap < tr.UNSATURATED).sum()),
        tr.UNSATURATED, ref.loss64))
    assert (gap > tr.SATURATED).sum() >= n / 4 and (gap < tr.UNSATURATED).sum() >= n / 4
    assert gap.min() > tr.SATURATION_CLEAR                         # (train_referee.py says why no window may stand near z1 = z0)
    assert np.exp(np.float32(-tr.SATURATED)) == 0                  # float32 underflow: the losing score is exactly 0
    wrong = (ref.z64[:, 1] > ref.z64[:, 0]) != (ref.y != 0)
    for part in (gap > tr.SATURATED, gap < tr.UNSATURATED):        # both sides of dz = rising ? -s0 : s1 in both regimes
        assert (wrong & part).any() and (~wrong & part).any()
    assert 1.001 * ref.loss64 > gap[wrong].sum() > 0.999 * ref.loss64       # wrongly decided windows cost about |z1 - z0| each
    tr.accept(ref.g32, ref.loss32, ref, "float32 CPU chain, dense2 x {}".format(tr.SATURATION_GAIN), tol=tr.CHAIN_BOUND)


def test_cases_meet_the_share_branches_of_k_wgrad_conv():
    """from the shapes of CASES by the rule of wgrad_shares with the kernel file's WGRAD_MAX_PER: every conv layer meets several
    shares with a shorter last one, some layer a share of exactly WGRAD_MAX_PER tasks; k_wgrad_conv1 meets a window size that is no
    multiple of its eight runs"""
    max_per = tr.wgrad_max_per()
    assert tr.wgrad_shares(73, 19, 16) == [13, 13, 11] and tr.wgrad_shares(32, 8, 16) == [16] and tr.wgrad_shares(9, 128, 16) == [10, 10]
    shorter, full, several = set(), set(), set()
    for case in tr.CASES:
        for layer, shares in tr.layer_shares(case[2], case[3], max_per).items():
            print("{} x {} {}: {} tasks -> {}".format(case[2], case[3], layer, sum(shares), "/".join(map(str, shares))))
            assert all(1 <= s <= max_per for s in shares)
            if len(shares) > 1:
                several.add(layer)
            if shares[-1] < shares[0]:
                shorter.add(layer)
            if max_per in shares:
                full.add(layer)
    assert shorter == several == {"conv2", "conv3", "conv4"}
    assert full
    assert {case[2] * case[3] % 8 for case in tr.CASES} >= {0, 4, 6, 7}
    widths = {w for case in tr.CASES for w in (case[3] - 2, (case[3] - 2) // 2)}
    assert {33, 64, 128} <= widths                                 # 32 + 1 columns; whole numbers of 32-column tiles


def test_exact_zero_rule_rejects_what_it_should():
    ref = tr.referee(*tr.CASES[0], tr.DROP)
    counts = {k: int((ref.s64[k] == 0).sum()) for k in tr.TENSORS}
    print("elements without a nonzero term:", counts)
    assert all(counts[k] > 0 for k in ("conv2_w", "conv3_w", "conv4_w", "dense1_w"))
    assert all(np.all(ref.s64[k] >= 0) for k in tr.TENSORS)
    for k in ("conv3_w", "dense1_w"):
        bad = {t: ref.g64[t] for t in tr.TENSORS}
        bad[k] = ref.g64[k].copy()
        bad[k][tuple(np.argwhere(ref.s64[k] == 0)[0])] = 1e-30         # far below anything the per-tensor rule sees
        assert tr.errors(bad, ref.loss64, ref)[k] < 1e-20
        with pytest.raises(AssertionError, match="nonzero where every term is 0"):
            tr.accept(bad, ref.loss64, ref)
    tr.accept(ref.g64, ref.loss64, ref)


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
