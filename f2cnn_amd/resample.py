"""Recordings of any rate, PCM format and channel count brought to the model's rate on the device (f2_resample_batch):
scipy.signal.resample_poly's default filter and arithmetic, for a batch of files in one call. The filter is designed here, on
the host, exactly as resample_poly designs it; conversion, mixdown and the polyphase FIR run on the GPU."""
from math import gcd

import numpy as np

from . import _lib

# dtype of the samples as scipy.io.wavfile.read returns them -> pcm_format (24-bit files arrive left-justified in int32)
PCM_FORMATS = {np.dtype(np.uint8): _lib.PCM_U8, np.dtype(np.int16): _lib.PCM_I16, np.dtype(np.int32): _lib.PCM_I32,
               np.dtype(np.float32): _lib.PCM_F32, np.dtype(np.float64): _lib.PCM_F64}


def pcm_format(dtype):
    """The F2_PCM_* value of a sample dtype; ValueError for a dtype the device does not convert."""
    try:
        return PCM_FORMATS[np.dtype(dtype)]
    except (KeyError, TypeError):
        raise ValueError("samples of type {} cannot be resampled (uint8, int16, int32, float32 or float64)".format(dtype))


def design_resampler(rate_in, rate_out):
    """(up, down, half_len, taps) that take rate_in to rate_out: up / down = rate_out / rate_in reduced, and the filter
    scipy.signal.resample_poly(x, up, down) designs by default - firwin(2 half_len + 1, 1 / max(up, down), window=('kaiser', 5.0))
    * up with half_len = 10 max(up, down). Equal rates: (1, 1, 0, [1.0]), the conversion alone."""
    from scipy.signal import firwin
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError("sample rates must be positive")
    g = gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    if up == down == 1:
        return 1, 1, 0, np.ones(1, np.float64)
    max_rate = max(up, down)
    half_len = 10 * max_rate
    taps = firwin(2 * half_len + 1, 1.0 / max_rate, window=('kaiser', 5.0)).astype(np.float64)
    taps *= up
    return up, down, half_len, taps


def resample_arrays(arrays, rate_in, rate_out, channel=-1, ctx=None):
    """The arrays - samples of ONE dtype and channel count, shaped (n,) or (n, channels) - as mono float64 in int16 units at
    rate_out, in one device call: a list of (ceil(n up / down),) float64 arrays. channel: the channel to keep, -1 for the mean."""
    arrays = [np.asarray(a) for a in arrays]
    if not arrays:
        return []
    if len({a.dtype for a in arrays}) != 1:
        raise ValueError("the arrays of one call must share a sample type")
    fmt = pcm_format(arrays[0].dtype)
    if any(a.ndim not in (1, 2) for a in arrays):
        raise ValueError("samples must be shaped (n,) or (n, channels)")
    counts = {1 if a.ndim == 1 else a.shape[1] for a in arrays}
    if len(counts) != 1:
        raise ValueError("the arrays of one call must share a channel count")
    channels = counts.pop()
    if channels < 1 or not -1 <= channel < channels:
        raise ValueError("channel {} of {}".format(channel, channels))
    ctx = ctx or _lib.default_context()
    up, down, half_len, taps = design_resampler(rate_in, rate_out)
    offsets = np.zeros(len(arrays) + 1, np.int64)
    offsets[1:] = np.cumsum([a.shape[0] for a in arrays])
    flat = np.ascontiguousarray(np.concatenate([a.reshape(a.shape[0], channels) for a in arrays]))
    out = np.empty(sum(_lib.resampled_length(a.shape[0], up, down) for a in arrays), np.float64)
    out_offsets = ctx.resample_batch(flat, fmt, channels, channel, offsets, len(arrays), up, down, taps, half_len, out, _lib.MEM_HOST)
    assert out_offsets[-1] == len(out)
    return [out[out_offsets[b]:out_offsets[b + 1]] for b in range(len(arrays))]
