"""Mixing matrices for `cnn smearsweep` (scripts/CNN/Evaluating.py: EvaluateSmearSweep; the device side is
f2_channel_mix_levels of include/f2cnn_hip.h, which takes (C, C) float64 matrices of up to MAX_CHANNELS channels: W[c][c'] is the
weight of input channel c' in output channel c). Both builders work on linear envelope amplitude and give non-negative weights
whose rows sum to 1: positive envelopes stay positive and a flat envelope stays flat.

SmearMatrix  channel interaction: a Gaussian spread, in ERB, on the scale the filterbank is spaced on
BandMatrix   a reduced number of bands: the N-band vocoder, every channel of a band replaced by the band's mean
"""
import math

import numpy

from ._lib import SMEAR_MAX_CHANNELS as MAX_CHANNELS
from .gammatone.filters import _EAR_Q, _MIN_BW


def erb_number(freqs):
    """E(f) = EarQ ln(f + EarQ minBW), the scale gammatone/filters.py spaces the centre frequencies on: one unit is one ERB"""
    return _EAR_Q * numpy.log(numpy.asarray(freqs, dtype=numpy.float64) + _EAR_Q * _MIN_BW)


def channel_spacing(centre_freqs):
    """the smallest distance between neighbouring channels in ERB (0.233 for 128 channels from 100 Hz to 8 kHz); inf for one"""
    e = erb_number(centre_freqs).reshape(-1)
    return float(numpy.abs(numpy.diff(e)).min()) if len(e) > 1 else math.inf


def SmearMatrix(centre_freqs, erbs):
    """Channel interaction with a spread of `erbs` ERB: W[c][c'] = exp(-((E_c - E_c') / erbs)^2 / 2) with E = erb_number of the
    channels' centre frequencies (ascending or descending), exactly 0 where |E_c - E_c'| > 4 erbs, every row divided by its sum.
    A spread below a quarter of the channel spacing gives the identity exactly. ValueError for a spread that is not finite and
    positive, for centre frequencies that are not strictly monotonic, or for more than MAX_CHANNELS channels."""
    erbs = float(erbs)
    if not (math.isfinite(erbs) and erbs > 0):
        raise ValueError("the spread must be finite and positive (ERB), not {!r}".format(erbs))
    e = erb_number(centre_freqs).reshape(-1)
    C = len(e)
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError("{} channels (1 to {})".format(C, MAX_CHANNELS))
    steps = numpy.diff(e)
    if C > 1 and not (numpy.isfinite(e).all() and ((steps > 0).all() or (steps < 0).all())):
        raise ValueError("the centre frequencies must be finite and strictly ascending or descending")
    if erbs < channel_spacing(centre_freqs) / 4:
        return numpy.eye(C, dtype=numpy.float64)
    d = e[:, None] - e[None, :]
    W = numpy.where(numpy.abs(d) > 4 * erbs, 0.0, numpy.exp(-0.5 * (d / erbs) ** 2))
    return numpy.ascontiguousarray(W / W.sum(axis=1, keepdims=True))


def BandMatrix(C, bands):
    """The N-band vocoder on C channels: numpy.array_split(arange(C), bands) groups neighbouring channels into `bands` groups,
    W[c][c'] = 1 / len(group) inside a group and 0 elsewhere. bands == C is the identity. ValueError unless 1 <= bands <= C <=
    MAX_CHANNELS."""
    C, bands = int(C), int(bands)
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError("{} channels (1 to {})".format(C, MAX_CHANNELS))
    if not 1 <= bands <= C:
        raise ValueError("{} bands of {} channels (1 to {})".format(bands, C, C))
    W = numpy.zeros((C, C), numpy.float64)
    for group in numpy.array_split(numpy.arange(C), bands):
        W[group[0]:group[-1] + 1, group[0]:group[-1] + 1] = 1.0 / len(group)
    return W
