"""What the recorded-masker tests share (tests/test_gpu_masker_*.py, tests/test_gpu_input_batch_masked.py): the utterance lengths,
two sets of four recordings with five levels each, and a NumPy restatement of the header's contract - the start of a segment from
Philox4x32-10 (the restatement of tests/test_gpu_shaped_noise.py, which is held against the published known answers), the cyclic
segment, and the mix."""
import math

import numpy as np

import f2cnn_oracle as orc
import speechlike
from f2cnn_amd import _lib
from test_gpu_shaped_noise import philox4x32_10

C, RADIUS, STEP = 128, 5, 160
# empty, a single sample, both sides of the 1024-thread stride of the sum, one window (n = 11 * step + 1), a few thousand
LENGTHS = (0, 1, 1023, 1024, 1025, 1761, 4000)
B = len(LENGTHS)
SEED = 0x1234_5678_9ABC
FILL = 0x5A
STREAM = _lib.MASKER_STREAM
SUM_THREADS = _lib.MASKER_SUM_THREADS


def _recording(seed, n):
    return np.random.default_rng([77, seed]).standard_normal(n) * 900.0


def _late(n, quiet):
    m = _recording(6, n)
    m[:quiet] = 0.0
    return m


# name -> (recordings, masker_of, snr_db): K = 5 levels over R = 4 recordings, two levels on one recording
SETS = {
    # a constant; hundreds of wraps; wraps for the long rows only; wraps only when the start is near the end (two levels)
    "wraps": ([np.array([-321.5]), _recording(1, 7), _recording(2, 1000), _recording(3, 5000)], (0, 1, 2, 3, 3), (10.0, -3.0, 20.0, 0.0, 6.0)),
    # a silent recording; one that is zero over its first 4500 of 5000 samples (two levels); one that wraps late; a short one
    "silent": ([np.zeros(300), _late(5000, 4500), _recording(4, 5000), _recording(5, 7)], (0, 1, 1, 2, 3), (5.0, 12.0, -6.0, 3.0, 0.0)),
}
K = 5


def ragged_waves(lengths=LENGTHS, seed=40):
    waves = [speechlike.make(seed + i, n, "syllables")[0] if n == 4000 else orc.synth_utterance(seed + i, n) for i, n in enumerate(lengths)]
    offsets = np.zeros(len(lengths) + 1, np.int64)
    offsets[1:] = np.cumsum(lengths)
    return np.concatenate(waves).astype(np.int16), offsets


def start_of(seed, r, utt, M):
    """((w1 << 32) | w0) mod M of Philox4x32-10(counter (r, 0x4D41534B, 0, utt), key (seed & 0xffffffff, seed >> 32))"""
    w0, w1, _, _ = philox4x32_10((r, STREAM, 0, utt), (seed & 0xFFFFFFFF, seed >> 32))
    return ((int(w1) << 32) | int(w0)) % int(M)


def segment(recording, start, n):
    return recording[(start + np.arange(n, dtype=np.int64)) % len(recording)]


def mixed(clean, gain, recording, start):
    """clean + gain * m, product and sum rounded separately; the clean samples themselves where gain is 0"""
    clean = np.asarray(clean, dtype=np.float64)
    if gain == 0.0:
        return clean.copy()
    return clean + gain * segment(recording, start, len(clean))


def gain_of(sigma, recording, start, n):
    """(sigma / sqrt(fsum(m^2) / n), its relative tolerance): the longest chain of additions of the fixed-order sum is ceil(n / 1024)
    in a thread, 6 in the wave's shuffles and 16 over the waves; 16 ulp cover the division, the square root and the device's sqrt"""
    if n == 0 or sigma == 0.0:
        return 0.0, 0.0
    m = segment(recording, start, n)
    P = math.fsum(float(v) * float(v) for v in m)
    if P == 0.0:
        return 0.0, 0.0
    return sigma / math.sqrt(P / n), (math.ceil(n / SUM_THREADS) + 22 + 16) * 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def ptr(a):
    return None if a is None else a.ctypes.data
