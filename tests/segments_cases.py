"""The inputs the GPU tests of the decoding stages share (tests/test_gpu_decision_*.py, tests/test_gpu_interval_tally.py), and the
condition they must meet, which tests/test_segments_host.py asserts on the CPU: every logit_scale * logit of the random streams stands
at least CLEAR away from a half-integer, so that the few ulp between the device's log and NumPy's (about 1e-9 at scale 2^16) cannot
move an emission and every comparison can be exact."""
import numpy as np

import segments_referee as ref
from f2cnn_amd import _lib

T = _lib.PATH_TILE
# rows per utterance of the ragged call: around a wave, around a tile, several tiles, and one utterance whose tile products cross the
# chunking of the per-utterance scan by one row
ROWS = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, _lib.PATH_SCAN_CHUNK * T + 1)
WO = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int64)
SCALES = (1.0, 37.5, 65536.0)
CLEAR = 1e-6
SEED = 114
# (logit_scale, penalty): 0, 1, a mid value and 2^40 at the scale the command line uses; 0 and a mid value at the others
CASES = [(65536.0, 0), (65536.0, 1), (65536.0, 3 * 65536), (65536.0, 1 << 40), (1.0, 0), (1.0, 2), (37.5, 0), (37.5, 90)]

_cache = {}


def random_scores():
    """(n, 2) float32 = (1 - p, p), p uniform in [0, 1), as tests/test_gpu_score_track.py builds them"""
    if "scores" not in _cache:
        p = np.random.default_rng(SEED).random(int(WO[-1])).astype(np.float32)
        _cache["scores"] = np.ascontiguousarray(np.stack([np.float32(1) - p, p], axis=1))
    return _cache["scores"]


def clearance(scores):
    """the smallest distance of logit_scale * logit from a half-integer over SCALES"""
    l = ref.logits(scores)
    return min(float(np.abs((s * l) % 1.0 - 0.5).min()) for s in SCALES)


def adversarial():
    """(scores, window_offsets, names): streams that hit every tie rule, the clip, a NaN, and q = 0 rows at tile edges"""
    rng = np.random.default_rng(SEED + 1)
    n = 2 * T + 1
    half = np.full(n, 0.5, np.float32)
    alt = np.where(np.arange(n) % 2 == 0, np.float32(0.9), np.float32(0.1)).astype(np.float32)
    sat = (rng.random(n) < 0.5).astype(np.float32)                       # 0 / 1: both sides of the clip
    nan = rng.random(n).astype(np.float32)
    nan[[0, 5, T, n - 1]] = np.nan
    edges = rng.random(n).astype(np.float32)
    edges[[0, T - 1, T, T + 1, 2 * T - 1, 2 * T]] = 0.5
    # alternating exact values whose sums tie again and again: +a, -a, ... with zeros in between
    walk = np.tile(np.array([0.75, 0.5, 0.25, 0.5], np.float32), n // 4 + 1)[:n]
    ps = [half, alt, sat, nan, edges, walk]
    scores = np.concatenate([np.stack([np.float32(1) - p, p], axis=1) for p in ps]).astype(np.float32)
    scores[n * 3 + 7, 0] = np.nan                                         # (a NaN in the other column too)
    wo = np.arange(len(ps) + 1, dtype=np.int64) * n
    return np.ascontiguousarray(scores), wo, ("half", "alternating", "saturated", "nan", "edges", "walk")


def reference(kind, logit_scale, penalty):
    """(q, path, value) of the referee for the random ragged call or the adversarial one, computed once"""
    key = (kind, logit_scale, penalty)
    if key not in _cache:
        scores, wo = (random_scores(), WO) if kind == "random" else adversarial()[:2]
        qkey = (kind, logit_scale)
        if qkey not in _cache:
            _cache[qkey] = ref.emissions(scores, logit_scale)
        path, value = ref.decision_path(_cache[qkey], wo, penalty)
        _cache[key] = (_cache[qkey], path, value)
    return _cache[key]
