"""A labelled corpus of WAV files for the tests of `cnn train --from-wav` (tests/test_gpu_train_from_wav.py,
tests/test_train_from_wav_cli.py): the waveform twin of tests/test_training.py's synthetic_windows. Every file is 16 000 samples of
seeded Gaussian noise in eight 2000-sample segments; inside a segment the amplitude ramps from 500 to 4000 (sign 1, rising) or back
(sign 0), and the segment's one centre sits in its middle, so that a window of the default configuration (11 rows 160 samples
apart, reach 800) stays inside its segment."""
import os

import numpy as np

SEGMENT, SEGMENTS = 2000, 8
N = SEGMENT * SEGMENTS


def make_file(seed):
    """(int16 samples, centres, signs) of one file"""
    rng = np.random.default_rng(seed)
    signs = rng.integers(0, 2, SEGMENTS).astype(np.uint8)
    ramp = np.linspace(500.0, 4000.0, SEGMENT)
    amp = np.concatenate([ramp if s else ramp[::-1] for s in signs])
    wave = np.clip(rng.standard_normal(N) * amp, -32000, 32000).astype(np.int16)
    return wave, np.arange(SEGMENTS, dtype=np.int64) * SEGMENT + SEGMENT // 2, signs


def keys(n_train=16, n_test=6):
    return ["TRAIN/DR{}.M{:03d}0.SA1".format(1 + i % 4, i) for i in range(n_train)] + \
           ["TEST/DR{}.F{:03d}0.SX2".format(1 + i % 4, i) for i in range(n_test)]


def write(root=".", n_train=16, n_test=6, seed=100, shuffle=True):
    """resources/f2cnn/{TRAIN,TEST}/*.WAV and trainingData/label_data.csv under `root`, the CSV rows of the files interleaved (CSV
    order is not file order). Returns {key: (wave, centres, signs)}."""
    from scipy.io import wavfile
    files, rows = {}, []
    for i, key in enumerate(keys(n_train, n_test)):
        wave, centres, signs = files[key] = make_file(seed + i)
        path = os.path.join(root, "resources", "f2cnn", key + ".WAV")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        wavfile.write(path, 16000, wave)
        tt, rest = key.split("/")
        region, speaker, sentence = rest.split(".")
        rows += [(tt, region, speaker, sentence, "aa", int(tp), 0.5, 0.01, int(s)) for tp, s in zip(centres, signs)]
    if shuffle:
        # files interleaved, the rows of one file in their order
        order = np.random.default_rng(seed).permutation(len(rows))
        rows = [rows[j] for j in sorted(order, key=lambda j: (j % SEGMENTS, order[j]))]
    os.makedirs(os.path.join(root, "trainingData"), exist_ok=True)
    with open(os.path.join(root, "trainingData", "label_data.csv"), "w") as f:
        for r in rows:
            f.write(",".join(map(str, r)) + "\n")
    return files
