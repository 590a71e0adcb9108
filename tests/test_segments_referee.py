"""The referee of the decoding stages (tests/segments_referee.py) against enumeration of all 2^n paths: the sequential definition
reaches the optimum, its path attains it, and with penalty 0 the path is the sign of the emissions with the stated tie rule."""
import numpy as np

import segments_referee as ref


def cases():
    rng = np.random.default_rng(44)
    for i in range(3000):
        n = int(rng.integers(0, 11))
        spread = int(rng.choice([1, 2, 5, 40]))     # small spreads make ties common
        yield rng.integers(-spread, spread + 1, n).tolist(), i % 7


def test_viterbi_reaches_the_optimum_of_all_paths():
    seen_tie = 0
    for q, penalty in cases():
        x, value = ref.viterbi(q, penalty)
        assert len(x) == len(q) and set(x) <= {0, 1}
        assert value == ref.brute_force(q, penalty), (q, penalty)
        assert ref.objective(x, q, penalty) == value, (q, penalty, x)
        seen_tie += 0 in q
    assert seen_tie > 500


def test_penalty_zero_is_the_sign_of_the_emission():
    for q, _ in cases():
        x, _ = ref.viterbi(q, 0)
        for j, qj in enumerate(q):
            if qj != 0:
                assert x[j] == (qj > 0), (q, x)
            else:
                assert x[j] == (x[j + 1] if j + 1 < len(q) else 0), (q, x)   # the row after it; the last row is falling


def test_huge_penalty_is_a_constant_path():
    for q, _ in cases():
        x, value = ref.viterbi(q, 1 << 40)
        if q:
            assert x == [1 if sum(q) > 0 else 0] * len(q) and value == max(sum(q), 0)


def test_emissions_round_to_even_clip_and_zero_nans():
    s = np.array([[0.5, 0.5], [0.0, 1.0], [1.0, 0.0], [np.nan, 0.3], [0.3, np.nan], [2.0, -1.0]], np.float32)
    q = ref.emissions(s, 1.0)
    assert q.tolist() == [0, 16, -16, 0, 0, -16] and q.dtype == np.int32     # ln 1e7 = 16.118


def test_runs_and_tally_on_a_worked_example():
    wo = [0, 5, 5, 8]
    labels = np.array([1, 1, 0, 0, 1, 0, 0, 0], np.uint8)
    q = np.array([3, 4, -1, -2, 5, -7, 0, 1], np.int32)
    offsets, runs = ref.decision_runs(labels, q, wo)
    assert offsets.tolist() == [0, 3, 3, 4]
    assert runs.tolist() == [[0, 2, 1, 7], [2, 2, 0, -3], [4, 1, 1, 5], [0, 3, 0, -6]]
    # one set of three intervals; rows stand at 10, 13, 16, 19, 22
    t = ref.interval_tally(labels, labels, q, wo, [0, 3], [[0, 10], [10, 17], [17, 100]], 10, 3)
    assert t.tolist() == [[0, 0, 0, 0], [3, 2, 2, 6], [2, 1, 1, 3],
                          [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0],
                          [0, 0, 0, 0], [3, 0, 0, -6], [0, 0, 0, 0]]
