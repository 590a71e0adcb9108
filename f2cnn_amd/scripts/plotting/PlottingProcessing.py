"""Drop-in for the data side of the reference's ``scripts/plotting/PlottingProcessing.py``: gammatonegram pictures (the
envelopes of the gammatone filterbank, one image row per channel, replicated by its ERB ratio, log-normalised), with the VTR
formant tracks on top. The reference plots a (941, n) float64 image through matplotlib; here the envelopes are pooled to
`width` time columns and turned into LogNorm levels on the device (f2_envelope_picture / f2_gammatonegram_batch), and the
host only repeats rows, looks colours up and writes a PNG (f2cnn_amd/png.py) - matplotlib is not needed.

`start` / `end` are sample indices (the reference's docstrings say seconds, its code indexes with them)."""
import os

import numpy

from ... import _lib
from ...config import F2Config
from ...png import write_png

POOLS = {'mean': 0, 'max': 1}
MAX_ENVELOPE_BYTES = 2 << 30          # envelopes (8 * C * samples) one f2_gammatonegram_batch call may hold
# anchors of the colour ramp of levels 1..255 (dark violet -> blue -> teal -> green -> yellow), equally spaced
RAMP = ("#440154", "#3b528b", "#21918c", "#5ec962", "#fde725")


def ERBScale(f):
    """Equivalent rectangular bandwidth at centre frequency f (Hz), Moore and Glasberg's linear approximation."""
    return 24.7 * (4.37 * f * 0.001 + 1)


def GetNewHeightERB(matrix, CENTER_FREQUENCIES):
    """(height, ratios): image rows each channel of `matrix` takes when its row is repeated by the ratio of its ERB to the ERB
    of the lowest channel (the last centre frequency), rounded to the nearest integer (ties to even), and their sum."""
    cf = numpy.asarray(CENTER_FREQUENCIES, dtype=numpy.float64)
    ratios = numpy.rint(ERBScale(cf[:len(matrix)]) / ERBScale(cf[-1])).astype(numpy.int64)
    return int(ratios.sum()), [int(r) for r in ratios]


def ReshapeEnvelopesForSpectrogram(envelopes, CENTER_FREQUENCIES, start=0, end=None):
    """The (height, end - start) float64 image: every row of `envelopes` repeated by its ERB ratio, columns start .. end."""
    _, ratios = GetNewHeightERB(envelopes, CENTER_FREQUENCIES)
    image = numpy.repeat(numpy.asarray(envelopes, dtype=numpy.float64), ratios, axis=0)
    return image[:, start:end] if end is not None else image[:, start:]


def column_edges(m, width, s=0):
    """(lo, hi) int64 arrays: column x of a `width`-column picture of the samples [s, s + m) covers [lo[x], hi[x]) -
    lo = s + floor(x m / width), hi = s + floor((x + 1) m / width), and hi = lo + 1 where that is empty (m < width: the
    nearest sample is repeated). The definition f2_envelope_picture implements; m == 0 has no samples to cover."""
    x = numpy.arange(int(width), dtype=numpy.int64)
    lo = s + x * int(m) // int(width)
    hi = s + (x + 1) * int(m) // int(width)
    return lo, numpy.where(hi == lo, lo + 1, hi)


def colour_table():
    """(256, 3) uint8: level 0 (a pixel LogNorm masks) white, levels 1..255 a piecewise-linear ramp through RAMP, whose
    anchors sit at levels 1, 64.5, 128, 191.5 and 255."""
    anchors = numpy.array([[int(c[i:i + 2], 16) for i in (1, 3, 5)] for c in RAMP], dtype=numpy.float64)
    pos = (numpy.arange(1, 256) - 1) * (len(RAMP) - 1) / 254.0          # 0 .. 4 along the ramp
    seg = numpy.minimum(pos.astype(numpy.int64), len(RAMP) - 2)
    frac = (pos - seg)[:, None]
    table = numpy.full((256, 3), 255, numpy.uint8)
    table[1:] = numpy.rint(anchors[seg] * (1 - frac) + anchors[seg + 1] * frac).astype(numpy.uint8)
    return table


def formant_column(sample, start, end, width):
    """Picture column of a sample index: floor((sample - start) width / (end - start))."""
    return int(numpy.floor((sample - start) * width / float(end - start)))


def formant_row(f, height, FRAMERATE=16000, LOW_FREQ=100):
    """Picture row of a frequency on the linear axis LOW_FREQ (bottom row) .. FRAMERATE / 2 (row 0) the reference gives imshow
    as `extent`: round((height - 1) (fmax - f) / (fmax - LOW_FREQ))."""
    fmax = FRAMERATE / 2
    return int(numpy.rint((height - 1) * (fmax - f) / float(fmax - LOW_FREQ)))


def draw_formants(rgb, tracks, sampPeriod, FRAMERATE, start, end, LOW_FREQ=100):
    """Black formant tracks on the (H, W, 3) picture of the samples [start, end): frame j of a track (Hz) sits at sample
    j * sampPeriod * FRAMERATE / 1e6; consecutive frames are joined by a vertical run in the later frame's column. Frames
    outside the picture are skipped. Returns the number of frames drawn."""
    height, width = rgb.shape[:2]
    drawn = 0
    if end <= start:
        return drawn
    for track in tracks:
        previous = None
        for j, f in enumerate(track):
            col = formant_column(j * sampPeriod * FRAMERATE / 1e6, start, end, width)
            row = formant_row(f, height, FRAMERATE, LOW_FREQ)
            if not (0 <= col < width and 0 <= row < height):
                previous = None
                continue
            top, bottom = (min(previous, row), max(previous, row)) if previous is not None else (row, row)
            rgb[top:bottom + 1, col] = 0
            previous = row
            drawn += 1
    return drawn


def _bank(cfg=None):
    from ..processing.GammatoneFiltering import filterbank_from_config
    cfg = cfg or F2Config()
    cf, coefs = filterbank_from_config(cfg)
    return cfg, cf, numpy.ascontiguousarray(coefs, dtype=numpy.float64)


def _span(n, start, end):
    """[start, end) clipped to the n samples of a file, the way the reference's slice image[:, start:end] clips"""
    s = min(max(int(start), 0), n)
    e = n if end is None else min(max(int(end), s), n)
    return s, e


def PlotEnvelopeSpectrogram(matrix, CENTER_FREQUENCIES, LOW_FREQ=100, FRAMERATE=16000, start=0, end=None, width=1600,
                            pool='mean', ctx=None):
    """The (H, width) uint8 level image of a (C, n) envelope matrix in host memory: columns start .. end pooled to `width`
    columns and log-normalised by one f2_envelope_picture call, every channel row repeated by its ERB ratio. Level 0 = a
    pixel <= 0 (masked), 1..255 = LogNorm over the picture."""
    ctx = ctx or _lib.default_context()
    env = numpy.ascontiguousarray(matrix, dtype=numpy.float64)
    Cn, n = env.shape
    _, ratios = GetNewHeightERB(env, CENTER_FREQUENCIES)
    levels = numpy.zeros((1, Cn, int(width)), numpy.uint8)
    ctx.envelope_picture(env, numpy.array([0, n], numpy.int64), 1, Cn, numpy.array([_span(n, start, end)], numpy.int64),
                         width, POOLS[pool], None, levels, _lib.MEM_HOST)
    return numpy.repeat(levels[0], ratios, axis=0)


def _render_batch(ctx, cfg, cf, coefs, items, start, end, formantToPlot, width, pool, LPF, CUTOFF, outs):
    """One f2_gammatonegram_batch call for the loaded files `items` = [(filename, framerate, samples)], one PNG each."""
    from ..processing.EnvelopeExtraction import FFT_PRECISION
    from ..processing.FBFileReader import ExtractFBFile
    from ...gammatone import filters
    waves = [filters._wave_args(samples) for _, _, samples in items]
    dt = waves[0][1] if all(w[1] == waves[0][1] for w in waves) else _lib.WAVE_F64
    dtype = numpy.int16 if dt == _lib.WAVE_I16 else numpy.float64
    offsets = numpy.zeros(len(waves) + 1, numpy.int64)
    offsets[1:] = numpy.cumsum([w[0].shape[0] for w in waves])
    spans = numpy.array([_span(w[0].shape[0], start, end) for w in waves], numpy.int64)
    flat = numpy.concatenate([w[0].astype(dtype, copy=False) for w in waves])
    Cn = coefs.shape[0]
    levels = numpy.zeros((len(waves), Cn, int(width)), numpy.uint8)
    ctx.gammatonegram_batch(flat, dt, offsets, coefs, len(waves), Cn, bool(LPF), CUTOFF if LPF else 0.0, FFT_PRECISION, spans,
                            width, POOLS[pool], None, levels, _lib.MEM_HOST)
    _, ratios = GetNewHeightERB(levels[0], cf)
    table = colour_table()
    paths = []
    for b, (filename, framerate, _) in enumerate(items):
        rgb = table[numpy.repeat(levels[b], ratios, axis=0)]
        formants, sampPeriod = ExtractFBFile(os.path.splitext(filename)[0] + '.FB')
        if formants is not None:
            tracks = formants[:, :4].T
            if 0 < formantToPlot < 5:
                tracks = tracks[formantToPlot - 1:formantToPlot]
            draw_formants(rgb, tracks, sampPeriod, framerate, int(spans[b, 0]), int(spans[b, 1]), cfg.low_freq)
        os.makedirs(os.path.dirname(outs[b]) or '.', exist_ok=True)
        paths.append(write_png(outs[b], rgb))
    return paths


def _default_out(filename):
    return os.path.join('graphs', 'gtg', os.path.splitext(os.path.basename(filename))[0] + '.png')


def PlotEnvelopesAndFormantsFromFile(filename, start=0, end=None, formantToPlot=5, width=1600, pool='mean', LPF=False, CUTOFF=None,
                                     out=None):
    """The gammatonegram of one WAV file as a PNG (graphs/gtg/<basename>.png, or `out`), by one f2_gammatonegram_batch call;
    with <file>.FB next to it the VTR formant tracks are drawn on top (formantToPlot 1..4: that track, anything else: all
    four). Returns the path written."""
    from ..processing.GammatoneFiltering import GetArrayFromWAV
    cfg, cf, coefs = _bank()
    framerate, samples = GetArrayFromWAV(filename)
    return _render_batch(_lib.default_context(), cfg, cf, coefs, [(filename, framerate, samples)], start, end, formantToPlot, width,
                         pool, LPF, CUTOFF, [out or _default_out(filename)])[0]


def PlotGammatonegrams(files, start=0, end=None, formantToPlot=5, width=1600, pool='mean', LPF=False, CUTOFF=None, out=None):
    """`plot gtg`: a PNG per file of `files` (`out` names the PNG of a single file). The files of a batch share one
    f2_gammatonegram_batch call; a batch is closed before its envelopes (8 * C * samples) would pass 2 GiB. A file that
    cannot be read is reported and skipped, the exit status is then 2. Returns the JobReport (`paths`: the PNGs written)."""
    from ...iopipe import JobReport
    from ..processing.GammatoneFiltering import GetArrayFromWAV
    report = JobReport("plot gtg")
    report.paths = []
    cfg, cf, coefs = _bank()
    ctx = _lib.default_context()
    cap = MAX_ENVELOPE_BYTES // (8 * coefs.shape[0])      # samples of a batch
    files = list(files)
    if out is not None and len(files) != 1:
        raise ValueError("`out` names the picture of one file; {} files given".format(len(files)))

    def flush(items):
        if not items:
            return
        outs = [out or _default_out(name) for name, _, _ in items]
        for path, (name, rate, samples) in zip(_render_batch(ctx, cfg, cf, coefs, items, start, end, formantToPlot, width, pool,
                                                            LPF, CUTOFF, outs), items):
            report.paths.append(path)
            print("\t\t{:<50} -> {}  {}/{} Files".format(name, path, report.add(len(samples), rate), len(files)))

    items, held = [], 0
    for name in files:
        try:
            rate, samples = GetArrayFromWAV(name)
        except Exception as exc:          # a missing, corrupt or unsupported file: the other files still run
            report.fail(name, exc)
            continue
        if items and held + len(samples) > cap:
            flush(items)
            items, held = [], 0
        items.append((name, rate, samples))
        held += len(samples)
    flush(items)
    report.finish()
    return report
