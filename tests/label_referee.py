"""The referee of the label-accuracy tests (tests/test_label_accuracy_cli.py, tests/test_gpu_label_accuracy.py): the rule of
f2_label_accuracy (include/f2cnn_hip.h; reference scripts/CNN/Evaluating.py:93-108) restated as it reads - every row against
every pair of consecutive labels - its hand-worked cases, and the inputs the two test files share. No GPU, no library."""
import os
import struct

import numpy as np

STEP = 160


def referee_loops(labels, T, s, origin, hop, step=STEP):
    """confusion[ref][pred] (2, 2) int64 of the rows `labels` (row j at t = origin + j * hop) against the label timepoints T and
    signs s: the rule word for word, a double loop over rows and consecutive label pairs."""
    conf = np.zeros((2, 2), np.int64)
    for j, label in enumerate(labels):
        t = origin + j * hop
        for k in range(len(T) - 1):
            before, after = int(T[k]), int(T[k + 1])
            if before < t < after and (t - before < step or after - t < step):
                ref = s[k] if t - before <= after - t else s[k + 1]
                conf[int(ref), int(label)] += 1
    return conf


def referee(labels, T, s, origin, hop, step=STEP):
    """referee_loops with the loop over the rows handed to NumPy, element by element (the loop over the pairs stays Python's):
    no search, no sorting, every row still meets every pair. For the utterances of tens of thousands of rows; held against
    referee_loops on the hand-worked cases and on the short utterances of the ragged batch."""
    labels = np.asarray(labels, dtype=np.int64)
    t = origin + hop * np.arange(len(labels), dtype=np.int64)
    conf = np.zeros((2, 2), np.int64)
    for k in range(len(T) - 1):
        before, after = int(T[k]), int(T[k + 1])
        counted = (before < t) & (t < after) & ((t - before < step) | (after - t < step))
        earlier = counted & (t - before <= after - t)
        later = counted & ~earlier
        for pred in (0, 1):
            conf[int(s[k]), pred] += int((earlier & (labels == pred)).sum())
            conf[int(s[k + 1]), pred] += int((later & (labels == pred)).sum())
    return conf


def one_row(t, T, s, label=1):
    """the referee on the single row at timepoint t: None when the row is not counted, else its reference sign"""
    conf = referee_loops([label], T, s, origin=t, hop=1)
    assert np.array_equal(conf, referee([label], T, s, origin=t, hop=1))
    assert conf.sum() in (0, 1) and conf[:, 1 - label].sum() == 0
    return None if conf.sum() == 0 else int(np.flatnonzero(conf[:, label])[0])


# (T, s, t, expected: None = not counted, else the reference sign), step = 160
HAND_CASES = [
    ([100, 300], [1, 0], 150, 1),
    ([100, 300], [1, 0], 200, 1),       # a tie goes to the earlier label
    ([100, 300], [1, 0], 201, 0),
    ([100, 300], [1, 0], 100, None),    # on a timepoint
    ([100, 300], [1, 0], 300, None),
    ([100, 300], [1, 0], 50, None),     # before the first label
    ([100, 300], [1, 0], 301, None),    # after the last
    ([100, 1000], [1, 0], 500, None),   # both neighbours a step or more away
    ([100, 1000], [1, 0], 259, 1),
    ([100, 1000], [1, 0], 260, None),   # 160 is not below the step
]


def check_hand_cases():
    for T, s, t, want in HAND_CASES:
        assert one_row(t, T, s) == want, (T, s, t, want)
        assert one_row(t, T, s, label=0) == want, (T, s, t, want)
    assert referee([1, 0, 1], [100], [1], 0, 50).sum() == 0 and referee([1, 0, 1], [], [], 0, 50).sum() == 0   # fewer than two labels


# ---- the ragged random batch of the GPU test ------------------------------------------------------------------------------------
ROWS = (0, 1, 255, 256, 257, 5000, 70000)
SET_SIZES = (0, 1, 2, 3, 40, 400, 2000)
GAPS = (1, 2, 159, 160, 161, 319, 320, 321, 1000)
CASES = [(hop, origin) for hop in (1, 7, 160) for origin in (0, 800)]
# One seed per case, found by search with the referee alone (ragged_condition): the pairs that can be counted are counted, under
# both reference signs. A set starts one gap after `origin`, so that the few hundred rows of the short utterances reach its labels
# at every hop; which gaps a two-label set needs for that depends on the hop, hence a seed per case.
SEEDS = {(1, 0): 15, (1, 800): 15, (7, 0): 1, (7, 800): 1, (160, 0): 1, (160, 800): 1}


def ragged_batch(hop, origin, seed=None):
    """labels (uint8, concatenated), window_offsets, ref_offsets, timepoints, signs of the batch for one case"""
    rng = np.random.default_rng(SEEDS[(hop, origin)] if seed is None else seed)
    wo = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int64)
    labels = rng.integers(0, 2, int(wo[-1])).astype(np.uint8)
    ro = np.concatenate([[0], np.cumsum(SET_SIZES)]).astype(np.int64)
    T = np.concatenate([origin + np.cumsum(rng.choice(GAPS, n)) for n in SET_SIZES]).astype(np.int64)
    s = rng.integers(0, 2, int(ro[-1])).astype(np.uint8)
    return labels, wo, ro, T, s


def ragged_referee(batch, hop, origin, pairs=range(len(ROWS))):
    labels, wo, ro, T, s = batch
    return {u: referee(labels[wo[u]:wo[u + 1]], T[ro[u]:ro[u + 1]], s[ro[u]:ro[u + 1]], origin, hop) for u in pairs}


def ragged_condition(conf):
    """every pair with two or more labels and at least one row has counted rows under both reference signs"""
    return all(conf[u][0].sum() > 0 and conf[u][1].sum() > 0 for u in conf if SET_SIZES[u] >= 2 and ROWS[u] >= 1)


# ---- the synthetic file of the end-to-end tests: a WAV with .FB / .PHN beside it, as tests/test_labels.py builds its corpus ------
def write_labelled_file(directory, wave_of, name="DR1.FSYN0.SA1", n=19200, frames=125):
    """<directory>/<name>.WAV (NIST SPHERE, 16 kHz, n samples from wave_of(n)), .FB (F2 a slow sinusoid between 1.1 and 1.9 kHz)
    and .PHN (one voiced phoneme over the whole file). Returns the WAV path."""
    from f2cnn_amd import wavio
    base = os.path.join(str(directory), name)
    wavio.write_sphere(base + ".WAV", 16000, wave_of(n))
    k = np.arange(frames)
    track = np.zeros((frames, 8))
    track[:, 0], track[:, 2], track[:, 3] = 0.5, 2.5, 3.5
    track[:, 1] = 1.5 + 0.4 * np.sin(2 * np.pi * 2.2 * k / 100.0)            # F2 in kHz, 2.2 Hz, a frame per 10 ms
    track[:, 4:] = 0.1
    with open(base + ".FB", "wb") as f:
        f.write(struct.pack('>iihh', frames, 100000, 32, 9) + track.astype('>f4').tobytes())
    with open(base + ".PHN", "w") as f:
        f.write("0 {} aa\n".format(n))
    return base + ".WAV"
