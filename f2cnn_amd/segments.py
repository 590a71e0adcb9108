"""`cnn eval --segments`: the host side of the decoder between the scores and the runs (the device side: f2_decision_path,
f2_decision_runs, f2_interval_tally, f2_eval_segments_batch in include/f2cnn_hip.h).

The rows of an evaluation are read as a two-state chain, falling / rising. A chain that stays in a state for `dwell` rows on
average leaves it with probability a = 1 / dwell per row, and the most probable state sequence given the network's scores maximises

    sum_j x_j * logit_j  -  ln((1 - a) / a) * (number of switches)

which is the objective f2_decision_path maximises exactly, on integers: logit_scale * logit_j rounded, the penalty rounded. What is
chosen here and not measured: the dwell time (--dwell, default three label frames) and the weight of a row's logit when rows
overlap (EmissionWeight). Nothing here is in the reference, which stops at the label per row."""
import math

import numpy

FIXED_POINT = 1 << 16           # integer units per nat
DEFAULT_DWELL_FRAMES = 3        # --dwell's default in label frames (STEP samples each): 30 ms at 16 kHz. A default, not a tuned value.


def DefaultDwellMs(STEP, framerate):
    return 1000.0 * DEFAULT_DWELL_FRAMES * STEP / framerate


def SwitchPenalty(dwell_ms, hop, framerate):
    """ln((1 - a) / a) nats, a = min(0.5, hop / dwell_samples): the price of a switch in a two-state chain whose expected dwell
    time is dwell_ms, seen every `hop` samples. A dwell of two rows or fewer costs nothing (a = 0.5)."""
    dwell_samples = float(dwell_ms) * framerate / 1000.0
    if not (dwell_samples > 0 and math.isfinite(dwell_samples)) or hop < 1:
        raise ValueError("the dwell time must be positive and finite, the hop at least 1 sample")
    a = min(0.5, hop / dwell_samples)
    return math.log((1.0 - a) / a)


def EmissionWeight(hop, STEP):
    """min(1, hop / STEP): rows closer together than one window row (STEP samples) share most of their input, so their logits are
    not independent evidence; the weight spreads one row's worth of evidence over the rows of a STEP. A stated heuristic, not a
    measurement: --segments-weight X replaces it."""
    if hop < 1 or STEP < 1:
        raise ValueError("hop and STEP must be at least 1 sample")
    return min(1.0, hop / float(STEP))


def Quantise(hop, STEP, framerate, dwell_ms=None, weight='auto'):
    """(logit_scale, penalty) as f2_decision_path takes them: logit_scale = 2^16 * weight, penalty = rint(2^16 * SwitchPenalty)."""
    w = EmissionWeight(hop, STEP) if weight in (None, 'auto') else float(weight)
    if not (0.0 < w <= 16.0):
        raise ValueError("the emission weight must lie in (0, 16]")
    dwell = DefaultDwellMs(STEP, framerate) if dwell_ms is None else dwell_ms
    return FIXED_POINT * w, int(round(FIXED_POINT * SwitchPenalty(dwell, hop, framerate)))


def PhonemeIntervals(phonemes):
    """(names, bounds (k, 2) int64) from PHNFileReader.ExtractPhonemes' [(phoneme, first sample, last sample)]: the half-open
    sample intervals [first, last) in ascending order, an interval cut where the next one starts before it ends."""
    rows = sorted(((int(a), int(b), str(name)) for name, a, b in (phonemes or []) if int(b) >= int(a) >= 0), key=lambda r: r[:2])
    bounds = numpy.array([[a, b] for a, b, _ in rows], numpy.int64).reshape(-1, 2)
    if len(bounds) > 1:
        bounds[:-1, 1] = numpy.minimum(bounds[:-1, 1], bounds[1:, 0])
    return [name for _, _, name in rows], bounds


def _ms(sample, framerate):
    return 1000.0 * sample / framerate


def RunsTable(what, runs, origin, hop, framerate, logit_scale, names=None, bounds=None):
    """Lines of the runs table of one utterance; runs (n, 4): first row, rows, label, sum of the emissions. Start and end are the
    centres of the run's first and last row in ms, the mean log-odds is that of the rows' (weighted) logits in nats."""
    lines = ["\t\t{}\ttransitions ({} runs)".format(what, len(runs)), "\t\tstart ms\tend ms\tduration ms\tdecision\tmean log-odds\tphonemes"]
    for j0, rows, label, total in numpy.asarray(runs, numpy.int64).reshape(-1, 4).tolist():
        first, last = origin + j0 * hop, origin + (j0 + rows - 1) * hop
        over = ""
        if names is not None:
            over = " ".join(name for name, (a, b) in zip(names, numpy.asarray(bounds).tolist()) if a <= last and b > first) or "-"
        lines.append("\t\t{:.1f}\t{:.1f}\t{:.1f}\t{}\t{:+.3f}\t{}".format(_ms(first, framerate), _ms(last, framerate), _ms(rows * hop, framerate),
                                                                      "rising" if label else "falling", total / (rows * logit_scale), over))
    return lines


def CombinePhonemeTally(names, tally):
    """(names in order of first appearance, (k, 4) int64): the interval tally summed over the intervals of the same name"""
    order, rows = [], {}
    for name, row in zip(names, numpy.asarray(tally, numpy.int64).reshape(-1, 4)):
        if name not in rows:
            order.append(name)
            rows[name] = numpy.zeros(4, numpy.int64)
        rows[name] += row
    return order, numpy.array([rows[name] for name in order], numpy.int64).reshape(-1, 4)


def PhonemeTable(what, names, tally, logit_scale):
    """Lines of the per-phoneme table: rows, % rising of the raw labels, % rising of the smoothed path, mean log-odds."""
    order, rows = CombinePhonemeTally(names, tally)
    lines = ["\t\t{}\tdecisions per phoneme".format(what), "\t\tphoneme\trows\t% rising raw\t% rising smoothed\tmean log-odds"]
    for name, (n, raw, smooth, total) in zip(order, rows.tolist()):
        if n:
            lines.append("\t\t{}\t{}\t{:.1f}\t{:.1f}\t{:+.3f}".format(name, n, 100.0 * raw / n, 100.0 * smooth / n, total / (n * logit_scale)))
        else:
            lines.append("\t\t{}\t0\t-\t-\t-".format(name))
    return lines
