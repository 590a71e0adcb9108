"""Recorded maskers for `cnn noisesweep --maskers` and `cnn train --augment-maskers` (scripts/CNN/Evaluating.py:
EvaluateNoiseSweep; scripts/CNN/Training.py; the device side is f2_masker_levels / f2_masker_pick of include/f2cnn_hip.h). A masker
is the recording itself - babble, a cafeteria, music, with the envelope modulations a Gaussian noise of its spectrum (noise.py's
`like:`) does not have: per utterance the library cuts a cyclic segment out of it and scales it to the level's SNR, so neither the
length nor the scale of the recording matters here. Not in the reference, whose only noise is white."""
import os

import numpy

from ._lib import MASKER_MAX_LEVELS as MAX_LEVELS, MASKER_MAX_RECORDINGS as MAX_RECORDINGS, MASKER_MAX_SAMPLES as MAX_SAMPLES


def LoadMasker(path, framerate, resample=False, ctx=None):
    """The recording `path` as mono float64 samples at `framerate`: any RIFF the `--resample` reader takes (8, 16, 32-bit integer,
    32 or 64-bit float PCM, one channel or more, which are averaged). A file at another rate goes through resample.resample_arrays
    (one device call) with resample=, and is a ValueError that names both rates without. ValueError too for an empty, an all-zero
    or a non-finite recording, and for one of more than MAX_SAMPLES samples."""
    from .wavio import read_audio
    rate, data = read_audio(path)
    data = numpy.asarray(data)
    if int(rate) != int(framerate):
        if not resample:
            raise ValueError("{}: the masker is at {} Hz, the recordings at {} Hz (resample it first, or --resample)".format(
                path, rate, int(framerate)))
        from .resample import resample_arrays
        m = resample_arrays([data], int(rate), int(framerate), channel=-1, ctx=ctx)[0] if len(data) else numpy.zeros(0)
    else:   # (int16 units, as the resampler gives them: an 8-bit file loses its offset of 128)
        m = data.astype(numpy.float64)
        if data.dtype == numpy.uint8:
            m = (m - 128.0) * 256.0
        elif data.dtype == numpy.int32:
            m = m / 65536.0
        elif data.dtype.kind == 'f':
            m = m * 32768.0
        elif data.dtype != numpy.int16:
            raise ValueError("{}: samples of type {} (8, 16 or 32-bit integer or 32 or 64-bit float PCM is needed)".format(path, data.dtype))
        if m.ndim == 2:
            m = m.mean(axis=1)
    m = numpy.ascontiguousarray(m, dtype=numpy.float64).reshape(-1)
    if not len(m) or not numpy.isfinite(m).all() or not numpy.abs(m).max() > 0:
        raise ValueError("{}: no finite, non-zero masker recording".format(path))
    if len(m) > MAX_SAMPLES:
        raise ValueError("{}: {} samples (at most {})".format(path, len(m), MAX_SAMPLES))
    return m


def MaskerName(path):
    """How a masker is printed and named in files: the stem of its file"""
    return os.path.splitext(os.path.basename(str(path)))[0]


def MaskerLevels(maskers, snrs):
    """The level grid of a masker sweep, masker-major over the SNRs: [(recording index, printed name, SNR)] - level
    m * len(snrs) + s is masker m at SNR s, named like 'babble 10dB' by the sweep. ValueError for no masker, an empty name, more
    than MAX_RECORDINGS recordings or more than MAX_LEVELS levels. Mirrors Evaluating.ColourLevels."""
    if isinstance(maskers, str):
        maskers = maskers.split(',')
    maskers = [str(m) for m in maskers]
    if not maskers or not all(maskers):
        raise ValueError("a masker sweep needs at least one recording")
    snrs = [float(v) for v in snrs]
    if not snrs:
        raise ValueError("maskers need the SNRs they are mixed in at")
    if len(maskers) > MAX_RECORDINGS:
        raise ValueError("at most {} masker recordings, not {}".format(MAX_RECORDINGS, len(maskers)))
    if len(maskers) * len(snrs) > MAX_LEVELS:
        raise ValueError("a noise sweep takes at most {} levels, not {} maskers x {} SNRs = {}".format(
            MAX_LEVELS, len(maskers), len(snrs), len(maskers) * len(snrs)))
    return [(r, MaskerName(m), v) for r, m in enumerate(maskers) for v in snrs]
