"""Room impulse responses for `cnn reverbsweep` (scripts/CNN/Evaluating.py: EvaluateReverbSweep; the device side is
f2_reverb_levels of include/f2cnn_hip.h, which takes a response of up to MAX_TAPS float64 taps).

SyntheticRIR  the Polack model: a unit direct path and exponentially decaying Gaussian noise behind it
LoadRIR       a measured response from a mono WAV file at the rate of the recordings, aligned to and normalised by its peak
"""
import math

import numpy

from ._lib import REVERB_MAX_TAPS as MAX_TAPS


def SyntheticRIR(t60, framerate, drr_db=0.0, seed=0, level=0):
    """The Polack model of a room with reverberation time t60 (seconds) at `framerate`: L = max(1, ceil(t60 * framerate)) float64
    taps, the time the tail takes to fall by 60 dB. h[0] = 1 is the direct path; h[k] = g * w[k] * 10^(-3 k / (t60 * framerate))
    for k >= 1 with w = numpy.random.default_rng([seed, level]).standard_normal(L), and g such that the tail's energy is
    10^(-drr_db / 10): drr_db is the direct-to-reverberant ratio. ValueError for a t60 that is not finite and positive or that needs
    more than MAX_TAPS taps."""
    t60, framerate = float(t60), float(framerate)
    if not (math.isfinite(t60) and t60 > 0):
        raise ValueError("t60 must be finite and positive, not {!r}".format(t60))
    if not (math.isfinite(framerate) and framerate > 0):
        raise ValueError("framerate must be finite and positive, not {!r}".format(framerate))
    if not math.isfinite(float(drr_db)):
        raise ValueError("drr_db must be finite, not {!r}".format(drr_db))
    span = t60 * framerate
    if span > MAX_TAPS:          # (before the ceil: a huge t60 never becomes an array length)
        raise ValueError("t60 = {:g} s at {:g} Hz needs {} taps (at most {})".format(t60, framerate, math.ceil(span), MAX_TAPS))
    L = max(1, int(math.ceil(span)))
    w = numpy.random.default_rng([int(seed), int(level)]).standard_normal(L)
    h = numpy.zeros(L, numpy.float64)
    h[0] = 1.0
    if L > 1:
        tail = w[1:] * numpy.power(10.0, -3.0 * numpy.arange(1, L, dtype=numpy.float64) / span)
        energy = float(numpy.dot(tail, tail))
        if energy > 0:
            h[1:] = tail * math.sqrt(10.0 ** (-float(drr_db) / 10.0) / energy)
    return h


def LoadRIR(path, framerate):
    """A measured impulse response: a mono WAV at `framerate` (another rate or more channels: ValueError that names the file),
    as float64, everything before the tap of largest magnitude dropped - so that the wet signal stays aligned with the dry one -
    and divided by that tap. ValueError for a silent file or for more than MAX_TAPS remaining taps."""
    from .wavio import read_audio
    rate, data = read_audio(path)
    if int(rate) != int(framerate):
        raise ValueError("{}: the impulse response is at {} Hz, the recordings at {} Hz (resample it first)".format(
            path, rate, int(framerate)))
    data = numpy.asarray(data)
    if data.ndim != 1:
        raise ValueError("{}: the impulse response has {} channels (one is needed)".format(path, data.shape[1]))
    h = data.astype(numpy.float64)
    if not len(h) or not numpy.isfinite(h).all() or not numpy.abs(h).max() > 0:
        raise ValueError("{}: no finite, non-zero impulse response".format(path))
    peak = int(numpy.argmax(numpy.abs(h)))
    h = h[peak:] / h[peak]
    if len(h) > MAX_TAPS:
        raise ValueError("{}: {} taps from the peak on (at most {})".format(path, len(h), MAX_TAPS))
    return numpy.ascontiguousarray(h)
