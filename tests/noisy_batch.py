"""The small ragged batch the noise-per-utterance tests share (tests/test_gpu_noise_pick*.py, tests/test_gpu_trainer_render.py): windows
of 13 x 40 (the shape tests/test_gpu_trainer.py trains at), six utterances - a short one, an empty one without centres, a power of
two, an odd length and one 1 s row for the spectral route under ctx.options(spectral_min_rows=0) - three noise levels, and a level
per utterance in which every level and the clean one occur."""
import numpy as np

import f2cnn_oracle as orc
from f2cnn_amd import _lib

C, RADIUS, STEP = 40, 6, 4
R = 2 * RADIUS + 1
REACH = RADIUS * STEP
LENGTHS = (257, 1500, 0, 4096, 3001, 16000)
B = len(LENGTHS)
SNR = (20.0, 3.0, -3.0)
K = len(SNR)
LEVEL_OF = (0, 3, 1, 2, 3, 1)
SEED = 0x1234_5678_9ABC
FILL = 0x5A


def coefs():
    return orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))


def waves(dtype=_lib.WAVE_I16, lengths=LENGTHS, seed=60):
    """(flat samples, offsets): int16 from orc.synth_utterance, the float64 variant scaled by 0.37"""
    flat = np.concatenate([orc.synth_utterance(seed + i, n) for i, n in enumerate(lengths)]).astype(np.int16)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return (flat if dtype == _lib.WAVE_I16 else flat.astype(np.float64) * 0.37), offsets


def centers(lengths=LENGTHS, per=(3, 5, 2, 7, 4, 6), seed=11):
    """(centres per utterance, center_offsets): the first and the last legal centre of every utterance with room for a window, and
    some between them (the rule of tests/test_gpu_input_from_wav.py's make_centers)"""
    rng = np.random.default_rng(seed)
    cs = []
    for b, n in enumerate(lengths):
        k = per[b % len(per)]
        if n < 2 * REACH + 1:
            cs.append(np.zeros(0, np.int64))
            continue
        c = rng.integers(REACH, n - REACH, size=k)
        c[0], c[-1] = REACH, n - 1 - REACH
        cs.append(c.astype(np.int64))
    return cs, np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def ptr(a):
    return None if a is None else a.ctypes.data
