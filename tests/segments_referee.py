"""Referee of the decoding stages behind `cnn eval --segments` (include/f2cnn_hip.h: f2_decision_path, f2_decision_runs,
f2_interval_tally): the header's definitions written down step by step - the recurrence and the runs on Python ints, the tally by
NumPy masks - with nothing clever in them. The device code scans; this walks. tests/test_segments_referee.py holds it against enumeration of all paths."""
import itertools

import numpy as np

CLIP = 1e-7


def emissions(scores, logit_scale):
    """q_j = rint(logit_scale * (ln c(p1) - ln c(p0))) in float64, ties to even, 0 for a NaN; int32"""
    s = np.asarray(scores, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    bad = np.isnan(s).any(axis=1)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(s, CLIP), 1.0)
    c[bad] = 1.0
    q = np.rint(float(logit_scale) * (np.log(c[:, 1]) - np.log(c[:, 0])))
    q[bad] = 0.0
    return q.astype(np.int32)


def logits(scores):
    """the float64 log-odds the emissions round (NaN rows: 0)"""
    s = np.asarray(scores, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    bad = np.isnan(s).any(axis=1)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(s, CLIP), 1.0)
    c[bad] = 1.0
    return np.log(c[:, 1]) - np.log(c[:, 0])


def objective(x, q, penalty):
    return sum(int(qj) for xj, qj in zip(x, q) if xj) - int(penalty) * sum(1 for a, b in zip(x[1:], x[:-1]) if a != b)


def viterbi(q, penalty):
    """(path as a list of 0 / 1, optimum) of one utterance by the sequential definition, ties included"""
    q = [int(v) for v in q]
    n, P = len(q), int(penalty)
    if n == 0:
        return [], 0
    v0, v1 = 0, q[0]
    bp0, bp1 = [0] * n, [1] * n
    for j in range(1, n):
        bp0[j] = 0 if v0 >= v1 - P else 1      # a tie stays
        bp1[j] = 1 if v1 >= v0 - P else 0
        v0, v1 = max(v0, v1 - P), max(v1, v0 - P) + q[j]
    x = [0] * n
    x[n - 1] = 1 if v1 > v0 else 0             # a tie is falling
    for j in range(n - 1, 0, -1):
        x[j - 1] = bp1[j] if x[j] else bp0[j]
    return x, max(v0, v1)


def brute_force(q, penalty):
    """the optimum over all 2^n paths"""
    return max(objective(x, q, penalty) for x in itertools.product((0, 1), repeat=len(q))) if len(q) else 0


def decision_path(q, window_offsets, penalty):
    """(path uint8 (n), value int64 (U)) of a ragged batch of emissions"""
    wo = [int(v) for v in window_offsets]
    path = np.zeros(wo[-1], np.uint8)
    value = np.zeros(len(wo) - 1, np.int64)
    for u in range(len(wo) - 1):
        x, value[u] = viterbi(q[wo[u]:wo[u + 1]], penalty)
        path[wo[u]:wo[u + 1]] = x
    return path, value


def decision_runs(labels, q, window_offsets):
    """(run_offsets (U + 1), runs (n_runs, 4) int64: first row within the utterance, rows, label, sum of q)"""
    wo = [int(v) for v in window_offsets]
    lab = [1 if v else 0 for v in np.asarray(labels).tolist()]
    qq = [0] * len(lab) if q is None else [int(v) for v in np.asarray(q).tolist()]
    offsets, runs = [0], []
    for u in range(len(wo) - 1):
        j = wo[u]
        while j < wo[u + 1]:
            k = j
            while k < wo[u + 1] and lab[k] == lab[j]:
                k += 1
            runs.append((j - wo[u], k - j, lab[j], sum(qq[j:k])))
            j = k
        offsets.append(len(runs))
    return np.array(offsets, np.int64), np.array(runs, np.int64).reshape(-1, 4)


def interval_tally(labels, path, q, window_offsets, iv_offsets, iv_bounds, origin, hop):
    """(rows, 4) int64, utterance-major: rows, rising labels, rising path, sum of q of the rows with a <= origin + j hop < b"""
    wo = [int(v) for v in window_offsets]
    ivo = [int(v) for v in iv_offsets]
    b = np.asarray(iv_bounds, dtype=np.int64).reshape(-1, 2)
    lab = np.asarray(labels) != 0
    pth = None if path is None else np.asarray(path) != 0
    qq = None if q is None else np.asarray(q).astype(np.int64)
    R = len(ivo) - 1
    out = []
    for u in range(len(wo) - 1):
        r = u % R
        rows = slice(wo[u], wo[u + 1])
        t = int(origin) + int(hop) * np.arange(wo[u + 1] - wo[u], dtype=np.int64)
        for k in range(ivo[r], ivo[r + 1]):
            own = (t >= b[k, 0]) & (t < b[k, 1])
            out.append((int(own.sum()), int(lab[rows][own].sum()), 0 if pth is None else int(pth[rows][own].sum()),
                        0 if qq is None else int(qq[rows][own].sum())))
    return np.array(out, np.int64).reshape(-1, 4)
