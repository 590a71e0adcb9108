"""Noise colours for `cnn noisesweep --colours` (scripts/CNN/Evaluating.py: EvaluateNoiseSweep; the device side is
f2_shaped_noise_levels of include/f2cnn_hip.h, which filters its Gaussian deviates with up to MAX_TAPS float64 taps per level and
does not normalise them).

ColourFIR  a named colour: white, pink, brown or speech-shaped
LikeFIR    the long-term spectrum of a recording (a mono WAV at the rate of the evaluation): its Welch estimate, not its samples
LoadFIR    taps from a 1-D .npy file

Every filter handed out is float64 and has sum h^2 = 1: the expected noise power is then sigma^2, so an SNR means what it means
for the white sweep. The designed ones are linear-phase and of odd length."""
import math

import numpy

from ._lib import SHAPED_MAX_TAPS as MAX_TAPS

GRID = 8192                                    # points of the frequency grid the magnitudes are sampled on (rfftfreq(GRID))
COLOURS = ('white', 'pink', 'brown', 'speech')


def Magnitude(name, f):
    """|H| of the colour `name` at the frequencies f (Hz, float64 array):
        pink    max(f, 20)^-1/2         (-3 dB per octave in power)
        brown   max(f, 20)^-1           (-6 dB per octave)
        speech  1 from 100 to 500 Hz, (f / 100)^2 below 100 Hz, (f / 500)^-1.5 above 500 Hz (-9 dB per octave)
    `speech` is the usual simplification of the long-term average speech spectrum: a stated convention, not a fit to any corpus.
    `white` is 1 everywhere."""
    f = numpy.asarray(f, dtype=numpy.float64)
    if name == 'white':
        return numpy.ones_like(f)
    if name == 'pink':
        return numpy.maximum(f, 20.0) ** -0.5
    if name == 'brown':
        return numpy.maximum(f, 20.0) ** -1.0
    if name == 'speech':
        return numpy.where(f < 100.0, (f / 100.0) ** 2, numpy.where(f <= 500.0, 1.0, (numpy.maximum(f, 500.0) / 500.0) ** -1.5))
    raise ValueError("unknown noise colour {!r} (one of {})".format(name, ', '.join(COLOURS)))


def _check_taps(taps):
    if int(taps) != taps or taps < 1 or taps % 2 == 0:
        raise ValueError("a noise filter takes an odd, positive number of taps, not {!r}".format(taps))
    if taps > MAX_TAPS:
        raise ValueError("{} taps (at most {})".format(int(taps), MAX_TAPS))
    return int(taps)


def _normalised(h):
    return numpy.ascontiguousarray(h / math.sqrt(float(numpy.dot(h, h))))


def _design(mag, taps):
    """The recipe: the magnitude on rfftfreq(GRID) -> irfft (zero phase) -> the centre rotated to the middle -> the middle `taps`
    samples -> times numpy.hanning(taps + 2)[1:-1] -> sum h^2 = 1. The two halves are averaged, so the taps are symmetric to the
    bit."""
    h = numpy.roll(numpy.fft.irfft(mag, GRID), GRID // 2)
    half = taps // 2
    h = h[GRID // 2 - half:GRID // 2 + half + 1] * numpy.hanning(taps + 2)[1:-1]
    return _normalised(0.5 * (h + h[::-1]))


def ColourFIR(name, framerate, taps=1025):
    """The filter of the colour `name` (see Magnitude) at `framerate`: `taps` (odd, at most MAX_TAPS) float64 taps, linear-phase,
    sum h^2 = 1, by the recipe of _design. 'white' is [1.0] exactly, one tap whatever `taps` says. The speech shape is a stated
    convention (flat from 100 to 500 Hz, -9 dB per octave above), not a fit to any corpus."""
    framerate = float(framerate)
    if not (math.isfinite(framerate) and framerate > 0):
        raise ValueError("framerate must be finite and positive, not {!r}".format(framerate))
    if name not in COLOURS:
        raise ValueError("unknown noise colour {!r} (one of {})".format(name, ', '.join(COLOURS)))
    taps = _check_taps(taps)
    if name == 'white' or taps == 1:
        return numpy.ones(1, numpy.float64)
    return _design(Magnitude(name, numpy.fft.rfftfreq(GRID, 1.0 / framerate)), taps)


WELCH_FRAME, WELCH_HOP = 1024, 512


def WelchMagnitude(x):
    """sqrt of the Welch mean of |rfft|^2 over Hann frames of WELCH_FRAME samples, WELCH_HOP apart: WELCH_FRAME / 2 + 1 values"""
    x = numpy.asarray(x, dtype=numpy.float64)
    starts = range(0, len(x) - WELCH_FRAME + 1, WELCH_HOP)
    window = numpy.hanning(WELCH_FRAME)
    power = numpy.zeros(WELCH_FRAME // 2 + 1)
    for s in starts:
        power += numpy.abs(numpy.fft.rfft(x[s:s + WELCH_FRAME] * window)) ** 2
    return numpy.sqrt(power / max(len(starts), 1))


def LikeFIR(path, framerate, taps=1025):
    """A filter whose magnitude is the long-term spectrum of the recording `path`: a mono WAV at `framerate` (another rate or
    more channels: ValueError that names the file). The Welch magnitude (WelchMagnitude) is interpolated to the grid of the named
    colours and goes through the same recipe: `taps` taps, linear-phase, sum h^2 = 1. Only the spectrum is matched: the noise
    stays Gaussian and stationary. ValueError for a silent file or one shorter than a single frame of WELCH_FRAME samples."""
    from .wavio import read_audio
    taps = _check_taps(taps)
    rate, data = read_audio(path)
    if int(rate) != int(framerate):
        raise ValueError("{}: the noise recording is at {} Hz, the recordings at {} Hz (resample it first)".format(
            path, rate, int(framerate)))
    data = numpy.asarray(data)
    if data.ndim != 1:
        raise ValueError("{}: the noise recording has {} channels (one is needed)".format(path, data.shape[1]))
    if len(data) < WELCH_FRAME:
        raise ValueError("{}: {} samples, shorter than one frame of {}".format(path, len(data), WELCH_FRAME))
    mag = WelchMagnitude(data)
    if not numpy.isfinite(mag).all() or not mag.max() > 0:
        raise ValueError("{}: no finite, non-zero noise recording".format(path))
    if taps == 1:
        return numpy.ones(1, numpy.float64)
    grid = numpy.fft.rfftfreq(GRID, 1.0 / float(framerate))
    return _design(numpy.interp(grid, numpy.fft.rfftfreq(WELCH_FRAME, 1.0 / float(framerate)), mag), taps)


def LoadFIR(path):
    """Taps from a 1-D float .npy file, as float64, divided by sqrt(sum h^2). ValueError for an array that is not 1-D, empty,
    not finite, of zero energy or longer than MAX_TAPS."""
    h = numpy.load(path)
    if h.ndim != 1 or h.dtype.kind not in 'fiu':
        raise ValueError("{}: a 1-D array of real taps is needed, not {} of shape {}".format(path, h.dtype, h.shape))
    h = h.astype(numpy.float64)
    if not len(h) or not numpy.isfinite(h).all() or not numpy.dot(h, h) > 0:
        raise ValueError("{}: no finite, non-zero taps".format(path))
    if len(h) > MAX_TAPS:
        raise ValueError("{}: {} taps (at most {})".format(path, len(h), MAX_TAPS))
    return _normalised(h)


def FromSpec(spec, framerate, taps=1025):
    """One entry of --colours: a name of COLOURS, 'like:<recording.wav>' or 'fir:<taps.npy>'"""
    if spec.startswith('like:'):
        return LikeFIR(spec[5:], framerate, taps)
    if spec.startswith('fir:'):
        return LoadFIR(spec[4:])
    return ColourFIR(spec, framerate, taps)


def SpecName(spec):
    """How a colour is printed and named in files: the name itself, or the stem of the file behind like: / fir:"""
    import os
    if spec.startswith(('like:', 'fir:')):
        return os.path.splitext(os.path.basename(spec.split(':', 1)[1]))[0]
    return spec
