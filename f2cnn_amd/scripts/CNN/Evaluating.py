"""Drop-in for the hot-path part of the reference's ``scripts/CNN/Evaluating.py``: WAV -> filterbank ->
envelope -> every-sample 11xC windows -> normalise -> CNN -> rising/falling label per sample
(``EvaluateOneWavArray`` :42-87, ``EvaluateOneWavFile`` :116-135). The scores and labels are returned and saved next to the
WAV; the figure the reference ends in (:109-113) is made with ``figure=True``.

``figure=True`` (``cnn eval|evalnoise|evalrand --figure [--figure-width W]``) is that figure, ``scripts/plotting/PlottingCNN.py``:
the gammatonegram with the formant track and a rising / falling tick per decision, and below it the network's probability of
"rising" over time beside arctan of the formant's slope, its p-value and the phoneme boundaries. The evaluation then goes
through ``f2_eval_figure_batch``: filterbank and envelope run once for decisions and picture, and the decisions come down
reduced to the W (default 1600) columns of the picture. The PNG goes to ``graphs/FallingOrRising/<basename>.png`` (for
``evalnoise`` the basename of the noisy file) and the ``.npz`` gains ``figure_track`` (W, 5: rows, rising rows, mean / min / max
probability per column) and ``figure_span``. Formant, slope and phoneme overlays come from the source file's ``.FB`` / ``.PHN``
where they exist (not for a file whose rate differed under ``resample=``), the accuracy text from ``accuracy=``. Scores and
labels are bit for bit those without the flag; ``figure=False`` changes nothing.

``occlusion=True | (band, stride) | dict`` (``cnn eval|evalnoise|evalrand --occlusion [BAND[:STRIDE]] [--occlusion-rows
RBAND[:RSTRIDE]] [--occlusion-fill V]``; not in the reference) asks what the decisions rest on: every window is evaluated again
with each patch of ``OcclusionPatches`` - bands of channels, optionally bands of window rows as well - replaced by the fill
value, in the same device pass (``f2_eval_occlusion_batch``: the windows are expanded, evaluated and reduced on the device). Per
patch a table line is printed - Hz range, rows, label flips, mean and mean absolute change of P(rising) - the ``.npz`` gains
``occlusion_patches`` (K, 4), ``occlusion_fill``, ``occlusion_scores`` (n, K+1, 2), ``occlusion_summary`` (K, 4),
``occlusion_map`` (K, W, 4: rows, flips, mean d, mean |d| per time column), ``occlusion_span`` and ``occlusion_hz`` (K, 2), and
``graphs/Occlusion/<basename>.png`` shows the map under the gammatonegram (``PlottingCNN.RenderOcclusion``; W =
``figure_width``; not with row bands). ``evalrand`` also prints the table of the corpus. Scores and labels are level 0 of the
pass, bit for bit those without the flag; ``occlusion=None`` changes nothing.

``saliency=True | N`` (``cnn eval|evalnoise|evalrand --saliency [--saliency-bands N]``; not in the reference) asks the same
question with one backward pass instead of one forward pass per band: G = dP(rising)/dx for every cell of every normalised window,
on the device (``f2_eval_saliency_batch``; only sum_r G x and sum_r |G| per window and channel are kept). Per N channels (default
8) a table line is printed - Hz range, rows, the sums of the mean G x and of the mean |G| - the ``.npz`` gains ``saliency_map``
(C, W, 3: rows, mean G x, mean |G| per channel and time column), ``saliency_summary`` (C, 3) and ``saliency_span``, and
``graphs/Saliency/<basename>.png`` shows the G x map under the gammatonegram (``PlottingCNN.RenderSaliency``; W =
``figure_width``). At N = 8 the G x column is the first-order prediction of ``--occlusion 8:8`` (fill 0) with the sign reversed.
One map per run: not together with ``occlusion=``. Scores and labels are bit for bit those without the flag; ``saliency=None``
changes nothing.

``segments=True | dict(dwell_ms=, weight=)`` (``cnn eval|evalnoise|evalrand --segments [--dwell MS] [--segments-weight auto|X]``;
not in the reference) smooths the decisions into transitions with the two-state decoder of ``segments.py``, on the device
(``f2_eval_segments_batch``; beside a figure or a map the three stage calls on that pass's scores). The runs table is printed,
with the file's ``.PHN`` (for ``evalnoise`` the clean file's; not for a file whose rate differed under ``resample=``) the phoneme
table as well, with ``accuracy=`` a second accuracy line for the smoothed decisions, and the ``.npz`` gains the ``segments_*`` keys
of ``_write_segments``. Scores and labels are bit for bit those without it; ``segments=None`` changes nothing.

The three commands share the request (``_Request``), the evaluation of a group of files (``_evaluate_group``: an ``_Evaluated`` per
file) and the end of a file (``_finish_file``); a file's blocks come in the order of the paragraphs above.

``accuracy='reference'|'centre'`` (``cnn eval|evalnoise|evalrand|noisesweep --accuracy [MODE]``) is the end of the reference's
``EvaluateOneWavArray`` (:38-40, :92-108): the decisions held against the labels ``LabelDataGenerator.ExtractLabel`` derives
from the SOURCE file's ``.FB`` / ``.PHN``, counted on the device (``f2_label_accuracy``, where the rule is written out). A row
within a STEP of a label timepoint is counted and takes the sign of the nearer label. ``reference`` compares the row's index
times the hop with the label timepoint, as the reference does (its own TODO: the index is not the row's centre sample);
``centre`` compares the row's true centre sample, radius*STEP further on. The default, ``accuracy=None``, changes nothing.

``hop=N`` (``cnn eval|evalnoise|evalrand --hop N``; not in the reference) evaluates every N-th of those windows only -
row j is every-sample row j*N, bit for bit (``f2_eval_batch_strided``) - and the ``.F2CNN.npz`` then also holds ``hop`` and
``timepoints``, the centre sample of every row. ``hop=None`` is the reference's every-sample loop.

``resample=True`` (``cnn eval|evalnoise|evalrand|noisesweep --resample``; not in the reference) brings every file to
``F2Config().framerate`` and to one channel on the device before anything else sees it (``GetArraysFromWAVsResampled``:
``f2_resample_batch``, one call per (rate, sample type, channel count) of a group of files): the filterbank, STEP and a ``frame``
hop are then those of that rate whatever the file's, and the ``.npz`` files gain ``framerate`` and ``source_framerate``. A file
that already is at that rate, mono and int16 is passed through untouched, so its results are bit for bit those without the flag.
With ``accuracy=`` a file whose rate differed gets no accuracy: the timepoints of its ``.FB`` / ``.PHN`` count source samples.
``resample=False`` changes nothing: a file is evaluated at its own rate, as the reference does.

``EvaluateCutoffSweep`` (``cnn lpfsweep --file X.WAV --cutoffs 5,10,20,50,100``; not in the reference, whose route is one ``cnn eval
--lpf HZ`` per cutoff) evaluates a file at every envelope cutoff and unfiltered in one device pass (``f2_eval_cutoff_sweep``): the
filterbank and the Hilbert envelope run once, the low-pass of ``EnvelopeExtraction.py:39-67`` K times on the result, and
``<base>.lpfsweep.npz`` holds the decisions of every level and their agreement with the unfiltered ones.

``EvaluateReverbSweep`` (``cnn reverbsweep --file X.WAV --t60 0.2,0.4,0.8 [--rir room.wav]``; not in the reference) evaluates a file
convolved with every room impulse response - synthetic ones of the given reverberation times and / or measured ones
(``f2cnn_amd/reverb.py``) - and dry in one device pass (``f2_eval_reverb_sweep``: the convolution runs on the device, in float64),
and ``OutputWavFiles/reverb/<stem>.reverbsweep.npz`` holds the decisions of every level, their agreement with the dry ones and the
responses that were used."""
import collections
import os

import numpy

from ... import _lib
from ...config import F2Config
from ...gammatone import filters
from ...model import F2CNNModel, load_model
from ...segments import CombinePhonemeTally, PhonemeIntervals, PhonemeTable, Quantise, RunsTable
from ..processing.EnvelopeExtraction import FFT_PRECISION
from ..processing.GammatoneFiltering import GetArrayFromWAV, GetArraysFromWAVsResampled


def _step(framerate, cfg):
    return int(framerate * cfg.sampling_period * (1 / 1000000.))


def _save(out, scores, labels, hop, N, framerate, extra=None):
    """<base>.F2CNN.npz: scores and labels; with a hop also the hop and the centre sample of every row; `extra`: the
    accuracy keys of _accuracy_keys"""
    extra = extra or {}
    if hop is None:
        numpy.savez(out, scores=scores, labels=labels, **extra)
        return
    cfg = F2Config()
    timepoints = _lib.strided_timepoints(N, cfg.radius, _step(framerate, cfg), hop)
    assert len(timepoints) == len(labels)
    numpy.savez(out, scores=scores, labels=labels, hop=numpy.int64(hop), timepoints=timepoints, **extra)


# ---- files at the model's rate (resample=True) ------------------------------------------------------------------------
def _load(files, resample):
    """[(source framerate, framerate of the samples, samples)] of the files: as they are read, or with resample= at
    F2Config().framerate and one channel (GetArraysFromWAVsResampled: one device call per kind of file)"""
    if not resample:
        return [(fr, fr, w) for fr, w in (GetArrayFromWAV(file) for file in files)]
    framerate = F2Config().framerate
    return [(source, framerate, w) for source, w in GetArraysFromWAVsResampled(files, framerate)]


def _rate_keys(resample, framerate, source):
    """what an .npz gains with resample="""
    return dict(framerate=numpy.int64(framerate), source_framerate=numpy.int64(source)) if resample else {}


def _no_rate_accuracy(file, source, framerate):
    print("\t\t{}\tresampled from {} Hz to {} Hz, the labels of its .FB / .PHN count source samples: no accuracy".format(
        file, source, framerate))


# ---- accuracy against the VTR labels (reference scripts/CNN/Evaluating.py:38-40, 92-108) -----------------------------
ACCURACY_MODES = ('reference', 'centre')


def ReferenceLabels(wavFile):
    """(timepoints int64, signs uint8) of the rows LabelDataGenerator.ExtractLabel gives for the file, or None when its
    .FB / .PHN side files are missing or give no rows (the reference's `labels is None`, :39-40)."""
    from configparser import ConfigParser
    from ...config import CONFIG_NAME
    from ..processing.LabelDataGenerator import CSV_COLUMNS, ExtractLabel
    config = ConfigParser()
    config.read_dict({'CNN': {'FORMANT': '2', 'RADIUS': '5', 'RISK': '0.05', 'SAMPLING_PERIOD': '10000'}})   # configure.py's answers
    config.read(CONFIG_NAME)
    rows = ExtractLabel(wavFile, config)
    if not rows:
        return None
    t, s = CSV_COLUMNS.index('timepoint'), CSV_COLUMNS.index('sign')
    return (numpy.array([row[t] for row in rows], numpy.int64), numpy.array([row[s] for row in rows], numpy.uint8))


def _accuracy_origin(accuracy, radius, STEP):
    """the sample row 0 is compared at: 0 as in the reference, or the row's centre"""
    if accuracy not in ACCURACY_MODES:
        raise ValueError("accuracy must be None, 'reference' or 'centre', not {!r}".format(accuracy))
    return 0 if accuracy == 'reference' else radius * STEP


def _accuracy_of(confusion):
    """correct / counted of confusion matrices (..., 2, 2) [ref][pred]; NaN where nothing is counted (the reference divides
    by zero there)"""
    confusion = numpy.asarray(confusion)
    correct = numpy.trace(confusion, axis1=-2, axis2=-1).astype(numpy.float64)
    counted = confusion.sum(axis=(-2, -1)).astype(numpy.float64)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        return numpy.asarray(numpy.where(counted > 0, correct / counted, numpy.nan), numpy.float64)


def _confusions(ctx, labels, window_offsets, refs, accuracy, hop, STEP):
    """(U, 2, 2) int64 [utterance][ref][pred] of host labels (concatenated, utterance u in window_offsets[u] .. [u + 1])
    against refs, one (timepoints, signs) or None per reference set; utterance u is scored against refs[u % len(refs)] (nothing
    is counted against a None). One device pass (f2_label_accuracy)."""
    cfg = F2Config()
    sets = [r if r is not None else (numpy.zeros(0, numpy.int64), numpy.zeros(0, numpy.uint8)) for r in refs]
    ref_offsets = numpy.zeros(len(sets) + 1, numpy.int64)
    ref_offsets[1:] = numpy.cumsum([len(t) for t, _ in sets])
    return ctx.label_accuracy(labels, window_offsets, ref_offsets, numpy.concatenate([t for t, _ in sets]),
                              numpy.concatenate([s for _, s in sets]), _accuracy_origin(accuracy, cfg.radius, STEP),
                              1 if hop is None else hop, STEP, _lib.MEM_HOST)


def _no_side_files(file):
    print("\t\t{}\tno labels from .FB / .PHN side files: no accuracy".format(file))


def _accuracy_keys(confusion, accuracy):
    """what a per-file .F2CNN.npz gains"""
    return dict(accuracy=numpy.float64(_accuracy_of(confusion)), confusion=numpy.asarray(confusion, numpy.int64),
                accuracy_mode=numpy.str_(accuracy))


def _print_accuracy(what, confusion, accuracy):
    print("\t\t{}\taccuracy against the VTR labels ({}): {:.4f} ({} of {} counted rows)".format(
        what, accuracy, float(_accuracy_of(confusion)), int(numpy.trace(confusion)), int(confusion.sum())))


def _file_accuracy(file, labels, accuracy, hop, framerate, ctx=None, what=None):
    """The accuracy keys of one file's labels against the labels of `file`'s side files ({} without them), printed (as `what`)."""
    _accuracy_origin(accuracy, 0, 0)      # (the mode is checked before anything is read)
    ref = ReferenceLabels(file)
    if ref is None:
        _no_side_files(file)
        return {}
    confusion = _confusions(ctx or _lib.default_context(), labels, [0, len(labels)], [ref], accuracy, hop,
                            _step(framerate, F2Config()))[0]
    _print_accuracy(what or file, confusion, accuracy)
    return _accuracy_keys(confusion, accuracy)


def _scored_extra(file, labels, accuracy, hop, framerate, source, resample):
    """the keys a per-file .npz gains from accuracy= and resample="""
    extra = {}
    if accuracy is not None and source != framerate:
        _accuracy_origin(accuracy, 0, 0)
        _no_rate_accuracy(file, source, framerate)
    elif accuracy is not None:
        extra = _file_accuracy(file, labels, accuracy, hop, framerate)
    return dict(extra, **_rate_keys(resample, framerate, source))


# ---- transitions: the decisions smoothed by the two-state decoder (segments.py; not in the reference) -----------------------
def _segments_spec(segments):
    """segments= as the callers give it (True, or a dict with dwell_ms / weight / intervals) with every key present"""
    given = {} if segments is True else dict(segments)
    return dict(dwell_ms=given.get('dwell_ms'), weight=given.get('weight', 'auto'), intervals=given.get('intervals'))


def _segments_sets(intervals, B):
    """(iv_offsets (B + 1), iv_bounds (total, 2)): one interval set per utterance, empty where it has none"""
    sets = [numpy.zeros((0, 2), numpy.int64) if iv is None else numpy.asarray(iv, numpy.int64).reshape(-1, 2)
            for iv in (intervals if intervals is not None else [None] * B)]
    if len(sets) != B:
        raise ValueError("segments: one interval set (or None) per utterance")
    offsets = numpy.zeros(B + 1, numpy.int64)
    offsets[1:] = numpy.cumsum([len(iv) for iv in sets])
    return offsets, numpy.concatenate(sets).reshape(-1, 2)


def PhonemeIntervalsOf(wavFile):
    """(names, bounds (k, 2) int64) of the file's .PHN, or None without it"""
    from ..processing.PHNFileReader import ExtractPhonemes
    phn = os.path.splitext(wavFile)[0] + '.PHN'
    if not os.path.exists(phn):
        return None
    names, bounds = PhonemeIntervals(ExtractPhonemes(phn))
    return (names, bounds) if names else None


def _file_phonemes(file, source, framerate):
    """PhonemeIntervalsOf the file for its segments (None: no .PHN, or a resampled file, whose .PHN counts source samples)"""
    if source != framerate:
        print("\t\t{}\tresampled from {} Hz to {} Hz, its .PHN counts source samples: no phoneme table".format(file, source, framerate))
        return None
    return PhonemeIntervalsOf(file)


def _write_segments(what, seg, framerate, names):
    """Prints the runs table and, with the names of the file's phonemes, the phoneme table; returns the segments_* keys of the .npz.
    seg: an entry's dict of EvaluateWavArrays(segments=)."""
    cfg = F2Config()
    origin = cfg.radius * _step(framerate, cfg)
    bounds = seg['intervals']
    for line in RunsTable(what, seg['runs'], origin, seg['hop'], framerate, seg['logit_scale'], names, bounds):
        print(line)
    keys = dict(segments_path=seg['path'], segments_runs=seg['runs'], segments_run_offsets=numpy.array([0, len(seg['runs'])], numpy.int64),
                segments_value=numpy.int64(seg['value']), segments_logit_scale=numpy.float64(seg['logit_scale']),
                segments_penalty=numpy.int64(seg['penalty']), segments_hop=numpy.int64(seg['hop']))
    if names is not None:
        for line in PhonemeTable(what, names, seg['tally'], seg['logit_scale']):
            print(line)
        order, rows = CombinePhonemeTally(names, seg['tally'])
        keys.update(segments_phoneme_names=numpy.array(order), segments_phoneme_tally=rows)
    return keys


def _smoothed_accuracy(file, seg, accuracy, framerate, source):
    """the second accuracy line of accuracy= with segments=: f2_label_accuracy on the path; its keys ({}: nothing to score)"""
    if accuracy is None or source != framerate:
        return {}
    keys = _file_accuracy(file, seg['path'], accuracy, seg['hop'], framerate, what=file + " (smoothed)")
    return {'segments_' + k: v for k, v in keys.items() if k != 'accuracy_mode'}


# ---- the figure (reference scripts/CNN/Evaluating.py:109-113, scripts/plotting/PlottingCNN.py) ------------------------------
FIGURE_WIDTH = 1600


def _figure_path(stem):
    return os.path.join('graphs', 'FallingOrRising', stem + '.png')


def _formant_number():
    """FORMANT of configF2CNN.conf (configure.py's answer without the file)"""
    from configparser import ConfigParser
    from ...config import CONFIG_NAME
    config = ConfigParser()
    config.read_dict({'CNN': {'FORMANT': '2'}})
    config.read(CONFIG_NAME)
    return config.getint('CNN', 'FORMANT')


def _write_figure(file, stem, levels, track, N, framerate, source, extra):
    """graphs/FallingOrRising/<stem>.png from the levels (C, W) and the track (W, 5) of a file of N samples, with the overlays
    the side files of `file` give; returns the keys the .npz gains"""
    from ...png import write_png
    from ..plotting import PlottingCNN
    from ..plotting.PlottingProcessing import GetNewHeightERB
    from ..processing.FBFileReader import GetFormantFrequencies
    from ..processing.PHNFileReader import ExtractPhonemes
    cfg = F2Config()
    _, ratios = GetNewHeightERB(levels, filters.centre_freqs(framerate, cfg.nchannels, cfg.low_freq))
    formant = slope = phonemes = None
    sampPeriod = cfg.sampling_period
    base = os.path.splitext(file)[0]
    if source != framerate:
        print("\t\t{}\tresampled from {} Hz to {} Hz, its .FB / .PHN count source samples: figure without formant, slope "
              "and phonemes".format(file, source, framerate))
    else:
        if os.path.exists(base + '.FB'):
            formant, sampPeriod = GetFormantFrequencies(base + '.FB', _formant_number())
            slope = PlottingCNN.FormantSlopeTrack(formant, cfg.radius, framerate * sampPeriod / 1000000.)
        if os.path.exists(base + '.PHN'):
            phonemes = ExtractPhonemes(base + '.PHN')
    accuracy = (extra or {}).get('accuracy')
    if accuracy is not None and not numpy.isfinite(accuracy):
        accuracy = None
    rgb = PlottingCNN.RenderFigure(levels, ratios, track, (0, N), framerate, formant, sampPeriod, slope, phonemes, accuracy,
                                   cfg.low_freq)
    path = _figure_path(stem)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_png(path, rgb)
    print("\t\t{}\tfigure -> {}".format(file, path))
    return dict(figure_track=track, figure_span=numpy.array([0, N], numpy.int64))


# ---- the occlusion map (not in the reference): which channel bands the decisions rest on -------------------------------------
OCCLUSION_BAND, OCCLUSION_STRIDE = 8, 8


def _bands(size, band, stride):
    """[start, end) of the bands of `band` cells that start every `stride` cells along an axis of `size`: 1 + ceil(max(size - band,
    0) / stride) of them, the last clipped at `size`"""
    size, band, stride = int(size), int(band), int(stride)
    if size < 1 or band < 1 or stride < 1:
        raise ValueError("an occlusion band needs a size, a width and a stride of at least 1")
    count = 1 + -(-max(size - band, 0) // stride)
    return [(i * stride, min(i * stride + band, size)) for i in range(count)]


def OcclusionPatches(rows, channels, band, stride, row_band=None, row_stride=None):
    """(K, 4) int32 {r0, r1, c0, c1}, half-open: the patches of an occlusion map over (rows, channels) windows. Channel bands of
    `band` channels start at i * stride, the last clipped at `channels`; row bands likewise from row_band / row_stride (default:
    all rows, one band). Row band major."""
    row_bands = [(0, int(rows))] if row_band is None else _bands(rows, row_band, row_band if row_stride is None else row_stride)
    if int(rows) < 1:
        raise ValueError("an occlusion band needs a size, a width and a stride of at least 1")
    return numpy.array([(r0, r1, c0, c1) for r0, r1 in row_bands for c0, c1 in _bands(channels, band, stride)],
                       numpy.int32).reshape(-1, 4)


def _occlusion_spec(occlusion):
    """occlusion= as the evaluation functions take it - True, (band, stride) or a dict with any of band, stride, row_band,
    row_stride, fill - as a dict with all of them"""
    spec = dict(band=OCCLUSION_BAND, stride=OCCLUSION_STRIDE, row_band=None, row_stride=None, fill=0.0)
    if isinstance(occlusion, dict):
        unknown = set(occlusion) - set(spec)
        if unknown:
            raise ValueError("occlusion= does not know {}".format(sorted(unknown)))
        spec.update(occlusion)
    elif occlusion is not True:
        spec['band'], spec['stride'] = occlusion
    if not 0.0 <= float(spec['fill']) <= 1.0:
        raise ValueError("the occlusion fill must lie in [0, 1], the range of a normalised window")
    return spec


def CombineOcclusionSummaries(summaries):
    """The (K, 4) summary {rows, flips, mean d, mean |d|} of several files as one: counts summed, means weighted by rows (a file
    without rows, whose means are NaN, weighs nothing; no rows at all: NaN)."""
    summaries = numpy.asarray(summaries, dtype=numpy.float64).reshape(len(summaries), -1, 4)
    rows = summaries[..., 0]
    out = numpy.full(summaries.shape[1:], numpy.nan)
    out[:, 0], out[:, 1] = rows.sum(axis=0), summaries[..., 1].sum(axis=0)
    some = out[:, 0] > 0
    for c in (2, 3):
        weighted = numpy.where(rows > 0, rows * summaries[..., c], 0.0).sum(axis=0)
        out[some, c] = weighted[some] / out[some, 0]
    return out


def OcclusionTable(what, patches, hz, summary):
    """The lines of the table `--occlusion` prints: one per patch - Hz range, rows, flips, flips %, mean d, mean |d|"""
    lines = ["\t\t{}\tocclusion: change of P(rising) with a patch of the input blanked".format(what),
             "\t\t{:>17} {:>7} {:>9} {:>9} {:>8} {:>10} {:>10}".format("Hz", "w.rows", "rows", "flips", "flips %", "mean d", "mean |d|")]
    for (r0, r1, _, _), (f0, f1), (rows, flips, d, ad) in zip(patches, hz, summary):
        lines.append("\t\t{:>8.0f}-{:<8.0f} {:>7} {:>9d} {:>9d} {:>8.2f} {:>+10.6f} {:>10.6f}".format(
            min(f0, f1), max(f0, f1), "{}-{}".format(r0, r1 - 1), int(rows), int(flips), 100.0 * flips / rows if rows else float('nan'),
            d, ad))
    return lines


def _occlusion_path(stem):
    return os.path.join('graphs', 'Occlusion', stem + '.png')


def _write_occlusion(file, stem, occ, N, framerate, source):
    """The table of one file's occlusion pass `occ` (EvaluateWavArrays), graphs/Occlusion/<stem>.png when every patch spans all
    rows of the window, and the keys the .npz gains"""
    from ...png import write_png
    from ..plotting import PlottingCNN
    from ..plotting.PlottingProcessing import GetNewHeightERB
    from ..processing.FBFileReader import GetFormantFrequencies
    cfg = F2Config()
    patches, levels = occ['patches'], occ['levels']
    cf = numpy.asarray(filters.centre_freqs(framerate, levels.shape[0], cfg.low_freq), numpy.float64)
    hz = numpy.stack([cf[patches[:, 2]], cf[patches[:, 3] - 1]], axis=1)
    for line in OcclusionTable(file, patches, hz, occ['summary']):
        print(line)
    if ((patches[:, 0] == 0) & (patches[:, 1] == cfg.dots_per_input)).all():
        _, ratios = GetNewHeightERB(levels, cf)
        formant, sampPeriod = None, cfg.sampling_period
        base = os.path.splitext(file)[0]
        if source == framerate and os.path.exists(base + '.FB'):
            formant, sampPeriod = GetFormantFrequencies(base + '.FB', _formant_number())
        rgb = PlottingCNN.RenderOcclusion(levels, ratios, occ['map'], patches, (0, N), framerate, formant, sampPeriod, cfg.low_freq)
        path = _occlusion_path(stem)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        write_png(path, rgb)
        print("\t\t{}\tocclusion map -> {}".format(file, path))
    else:
        print("\t\t{}\tocclusion patches with row bands: table and .npz keys only, no picture".format(file))
    return dict(occlusion_patches=patches, occlusion_fill=numpy.float32(occ['fill']), occlusion_scores=occ['scores'],
                occlusion_summary=occ['summary'], occlusion_map=occ['map'], occlusion_span=numpy.array([0, N], numpy.int64),
                occlusion_hz=hz)


# ---- the saliency map (not in the reference): the input gradient of the decisions, per channel ---------------------------------
SALIENCY_BANDS = 8


def _saliency_bands(saliency):
    """saliency= as the evaluation functions take it - True, or the channels per line of the table - as that count"""
    bands = SALIENCY_BANDS if saliency is True else int(saliency)
    if bands < 1:
        raise ValueError("a saliency band needs at least 1 channel")
    return bands


def CombineSaliencySummaries(summaries):
    """The (C, 3) summary {rows, mean G x, mean |G|} of several files as one: rows summed, means weighted by rows (a file without
    rows, whose means are NaN, weighs nothing; no rows at all: NaN)."""
    summaries = numpy.asarray(summaries, dtype=numpy.float64).reshape(len(summaries), -1, 3)
    rows = summaries[..., 0]
    out = numpy.full(summaries.shape[1:], numpy.nan)
    out[:, 0] = rows.sum(axis=0)
    some = out[:, 0] > 0
    for c in (1, 2):
        weighted = numpy.where(rows > 0, rows * summaries[..., c], 0.0).sum(axis=0)
        out[some, c] = weighted[some] / out[some, 0]
    return out


def SaliencyTable(what, cf, summary, bands=SALIENCY_BANDS):
    """The lines of the table `--saliency` prints: one per `bands` channels - Hz range, rows, and the sums over the band's channels
    of the mean G x and of the mean |G| of `summary` (C, 3). cf: the channels' centre frequencies. The third column is the
    first-order prediction of what `--occlusion BANDS:BANDS` measures for the band with fill 0, with the sign reversed."""
    summary = numpy.asarray(summary, dtype=numpy.float64).reshape(-1, 3)
    lines = ["\t\t{}\tsaliency: gradient of P(rising) at the input, per band of {} channels".format(what, int(bands)),
             "\t\t{:>17} {:>9} {:>9} {:>12} {:>12}".format("Hz", "channels", "rows", "sum G x", "sum |G|")]
    for c0, c1 in _bands(len(summary), bands, bands):
        part = summary[c0:c1]
        lines.append("\t\t{:>8.0f}-{:<8.0f} {:>9} {:>9d} {:>+12.6f} {:>12.6f}".format(
            min(cf[c0], cf[c1 - 1]), max(cf[c0], cf[c1 - 1]), "{}-{}".format(c0, c1 - 1), int(part[0, 0]), part[:, 1].sum(),
            part[:, 2].sum()))
    return lines


def _saliency_path(stem):
    return os.path.join('graphs', 'Saliency', stem + '.png')


def _write_saliency(file, stem, sal, N, framerate, source):
    """The table of one file's saliency pass `sal` (EvaluateWavArrays), graphs/Saliency/<stem>.png, and the keys the .npz gains"""
    from ...png import write_png
    from ..plotting import PlottingCNN
    from ..plotting.PlottingProcessing import GetNewHeightERB
    from ..processing.FBFileReader import GetFormantFrequencies
    cfg = F2Config()
    levels = sal['levels']
    cf = numpy.asarray(filters.centre_freqs(framerate, levels.shape[0], cfg.low_freq), numpy.float64)
    for line in SaliencyTable(file, cf, sal['summary'], sal['bands']):
        print(line)
    _, ratios = GetNewHeightERB(levels, cf)
    formant, sampPeriod = None, cfg.sampling_period
    base = os.path.splitext(file)[0]
    if source == framerate and os.path.exists(base + '.FB'):
        formant, sampPeriod = GetFormantFrequencies(base + '.FB', _formant_number())
    rgb = PlottingCNN.RenderSaliency(levels, ratios, sal['map'], (0, N), framerate, formant, sampPeriod, cfg.low_freq)
    path = _saliency_path(stem)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_png(path, rgb)
    print("\t\t{}\tsaliency map -> {}".format(file, path))
    return dict(saliency_map=sal['map'], saliency_summary=sal['summary'], saliency_span=numpy.array([0, N], numpy.int64))


def EvaluateOneWavArray(wavArray, framerate, wavFileName=None, model='last_trained_model', LPF=False, CUTOFF=100,
                        CENTER_FREQUENCIES=None, FILTERBANK_COEFFICIENTS=None, ctx=None, return_envelopes=False, hop=None,
                        saliency=None):
    """Returns (scores (nb,2) float32, labels (nb,) uint8 [, envelopes (C,N) float64]); nb = N - 11*STEP, or with a hop
    ceil(nb / hop) rows, row j centred at sample radius*STEP + j*hop. With saliency= (True, or the channels per table line) the
    pass is EvaluateWavArrays' and the tuple ends in its saliency dict."""
    if saliency is not None:
        if return_envelopes:
            raise ValueError("the saliency pass does not return envelopes")
        return EvaluateWavArrays([wavArray], framerate, model=model, LPF=LPF, CUTOFF=CUTOFF,
                                 FILTERBANK_COEFFICIENTS=FILTERBANK_COEFFICIENTS, ctx=ctx, hop=hop, saliency=saliency)[0]
    if hop is not None and return_envelopes:
        raise ValueError("the strided evaluation (hop) does not return envelopes")
    ctx = ctx or _lib.default_context()
    cfg = F2Config()
    if FILTERBANK_COEFFICIENTS is None:
        CENTER_FREQUENCIES = filters.centre_freqs(framerate, cfg.nchannels, cfg.low_freq)
        FILTERBANK_COEFFICIENTS = filters.make_erb_filters(framerate, CENTER_FREQUENCIES)
    coefs = numpy.ascontiguousarray(FILTERBANK_COEFFICIENTS, dtype=numpy.float64)
    Cn = coefs.shape[0]
    if not isinstance(model, F2CNNModel):
        model = load_model(model)
    print("Applying filterbank...")
    if not LPF:
        print("Extracting Envelope...")
    else:
        print("Extraction Envelope with {}Hz Low Pass Filter...".format(CUTOFF))
    wave, dt = filters._wave_args(wavArray)
    N = wave.shape[0]
    STEP = _step(framerate, cfg)
    nb = max(int(N - cfg.dots_per_input * STEP), 0)
    if hop is not None:
        nb = _lib.strided_window_count(N, cfg.radius, STEP, hop)
    print("Generating input data for CNN...")
    print("INPUT SHAPE:", (nb, cfg.dots_per_input, Cn))
    scores = numpy.empty((nb, 2), numpy.float32)
    labels = numpy.empty(nb, numpy.uint8)
    env = numpy.empty((Cn, N), numpy.float64) if return_envelopes else None
    print("Evaluating the data with the pretrained model...")
    try:
        if hop is not None:
            got = ctx.eval_batch_strided(model.handle(ctx), wave, dt, numpy.array([0, N], numpy.int64), coefs, 1, Cn, bool(LPF),
                                         CUTOFF if LPF else 0.0, FFT_PRECISION, cfg.radius, STEP, hop, scores, labels,
                                         _lib.MEM_HOST)[1]
        else:
            got = ctx.eval_utterance(model.handle(ctx), wave, dt, N, coefs, Cn, bool(LPF), CUTOFF if LPF else 0.0,
                                     FFT_PRECISION, cfg.radius, STEP, env, scores, labels, _lib.MEM_HOST)
    except _lib.F2Error as e:
        if e.code == _lib.F2_ERR_NONPOSITIVE:
            raise ValueError("values must all be positive")
        raise
    assert got == nb
    return (scores, labels, env) if return_envelopes else (scores, labels)


# ---- batch / noise evaluation (reference scripts/CNN/Evaluating.py:138-221) -------------
class _Request(collections.namedtuple('_Request', 'hop device_hop figure_width map_width occlusion saliency segments')):
    """What a run asks of the evaluation beyond scores and labels, settled once from the keywords: the hop as given and as the
    device sees it (1 for None), the figure's width (None: no figure), the width of a map, and the occlusion spec
    (_occlusion_spec), the saliency bands (_saliency_bands) and the segments spec (_segments_spec), None where not asked for."""
    __slots__ = ()

    @classmethod
    def of(cls, hop=None, figure_width=None, map_width=None, occlusion=None, saliency=None, segments=None):
        if occlusion is not None and saliency is not None:
            raise ValueError("one map per pass: occlusion= or saliency=, not both")
        return cls(hop, 1 if hop is None else hop, None if figure_width is None else int(figure_width),
                   int(map_width or figure_width or FIGURE_WIDTH), None if occlusion is None else _occlusion_spec(occlusion),
                   None if saliency is None else _saliency_bands(saliency), None if segments is None else _segments_spec(segments))

    @classmethod
    def of_command(cls, hop, figure, figure_width, occlusion, saliency, segments):
        """the request of cnn eval / evalnoise / evalrand: one width for the figure and the maps"""
        return cls.of(hop, figure_width if figure else None, figure_width, occlusion, saliency, segments)

    @property
    def needs_pass(self):
        """something only the batch pass (_evaluate_arrays) makes"""
        return any(x is not None for x in (self.figure_width, self.occlusion, self.saliency, self.segments))


# one utterance of _evaluate_arrays; what was not asked for is None. levels, track: the figure's; occlusion, saliency, segments:
# the dicts EvaluateWavArrays documents
_Evaluated = collections.namedtuple('_Evaluated', 'scores labels levels track occlusion saliency segments')


def _evaluate_arrays(wavArrays, framerate, req, model, LPF, CUTOFF, FILTERBANK_COEFFICIENTS, ctx=None):
    """EvaluateWavArrays' device pass for the request `req`: an _Evaluated per utterance"""
    ctx = ctx or _lib.default_context()
    cfg = F2Config()
    if FILTERBANK_COEFFICIENTS is None:
        FILTERBANK_COEFFICIENTS = filters.make_erb_filters(framerate, filters.centre_freqs(framerate, cfg.nchannels,
                                                                                           cfg.low_freq))
    coefs = numpy.ascontiguousarray(FILTERBANK_COEFFICIENTS, dtype=numpy.float64)
    Cn = coefs.shape[0]
    if not isinstance(model, F2CNNModel):
        model = load_model(model)
    if not len(wavArrays):
        return []
    waves, dts = zip(*[filters._wave_args(w) for w in wavArrays])
    if len(set(dts)) != 1:
        raise ValueError("the utterances of one batch must share a sample type (int16 or float64)")
    B = len(waves)
    offsets = numpy.zeros(B + 1, numpy.int64)
    offsets[1:] = numpy.cumsum([w.shape[0] for w in waves])
    flat = numpy.concatenate(waves)
    STEP = _step(framerate, cfg)
    nbs = [max(int(w.shape[0] - cfg.dots_per_input * STEP), 0) for w in waves]
    if req.hop is not None:
        nbs = [_lib.strided_window_count(w.shape[0], cfg.radius, STEP, req.hop) for w in waves]
    n, W, H = sum(nbs), req.map_width, _lib.MEM_HOST
    scores = numpy.empty((n, 2), numpy.float32)
    labels = numpy.empty(n, numpy.uint8)
    levels = track = occ = sal = seg = got = None
    if req.segments is not None:
        seg_scale, seg_penalty = Quantise(req.device_hop, STEP, framerate, req.segments['dwell_ms'], req.segments['weight'])
        ivo, ivb = _segments_sets(req.segments['intervals'], B)
        seg = dict(path=numpy.empty(n, numpy.uint8), emissions=numpy.empty(n, numpy.int32), runs=numpy.empty((n, 4), numpy.int64),
                   tally=numpy.zeros((int(ivo[-1]), 4), numpy.int64))
        seg_wo = numpy.concatenate([[0], numpy.cumsum(nbs)]).astype(numpy.int64)
    try:
        front = (model.handle(ctx), flat, dts[0], offsets, coefs, B, Cn, bool(LPF), CUTOFF if LPF else 0.0, FFT_PRECISION, cfg.radius, STEP)
        if req.saliency is not None or req.occlusion is not None:
            if req.saliency is not None:
                sal = dict(bands=req.saliency, map=numpy.empty((B, Cn, W, 3), numpy.float64), summary=numpy.empty((B, Cn, 3), numpy.float64),
                           levels=numpy.zeros((B, Cn, W), numpy.uint8))
                got, _ = ctx.eval_saliency_batch(*front, req.device_hop, None, W, 0, sal['levels'], sal['map'], sal['summary'], scores,
                                                 labels, H)
            else:
                spec = req.occlusion
                patches = OcclusionPatches(cfg.dots_per_input, Cn, spec['band'], spec['stride'], spec['row_band'], spec['row_stride'])
                K = len(patches)
                occ = dict(patches=patches, fill=numpy.float32(spec['fill']), scores=numpy.empty((n, K + 1, 2), numpy.float32),
                           labels=numpy.empty((n, K + 1), numpy.uint8), map=numpy.empty((B, K, W, 4), numpy.float64),
                           summary=numpy.empty((B, K, 4), numpy.float64), levels=numpy.zeros((B, Cn, W), numpy.uint8))
                got, _ = ctx.eval_occlusion_batch(*front, req.device_hop, patches, occ['fill'], None, W, 0, occ['levels'], occ['map'],
                                                  occ['summary'], occ['scores'], occ['labels'], H)
                scores[...], labels[...] = occ['scores'][:, 0], occ['labels'][:, 0]
            if req.figure_width is not None:       # the figure beside a map: the map call's levels, the track of its scores
                levels = (sal or occ)['levels']
                whole = numpy.stack([offsets[:-1] * 0, numpy.diff(offsets)], axis=1)
                track = ctx.score_track(scores, labels, got, whole, cfg.radius * STEP, req.device_hop, W,
                                        numpy.empty((B, W, 5), numpy.float64), H)
        elif req.figure_width is not None:
            levels = numpy.zeros((B, Cn, req.figure_width), numpy.uint8)
            track = numpy.empty((B, req.figure_width, 5), numpy.float64)
            got, _ = ctx.eval_figure_batch(*front, req.device_hop, None, req.figure_width, 0, levels, track, scores, labels, H)
        elif seg is not None:
            got, seg['value'], seg['run_offsets'] = ctx.eval_segments_batch(
                *front, req.device_hop, seg_scale, seg_penalty, ivo, ivb, scores, labels, seg['path'], seg['emissions'], seg['runs'],
                seg['tally'], H)
        elif req.hop is not None:
            got = ctx.eval_batch_strided(*front, req.hop, scores, labels, H)
        else:
            ctx.eval_batch(*front, scores, labels, H)
        assert got is None or list(numpy.diff(got)) == nbs
        if seg is not None and 'value' not in seg:     # beside a figure or a map: the three stage calls on its scores
            seg['value'] = ctx.decision_path(scores, seg_wo, seg_scale, seg_penalty, seg['path'], H, emissions=seg['emissions'])
            seg['run_offsets'] = ctx.decision_runs(seg['path'], seg['emissions'], seg_wo, seg['runs'], len(seg['runs']), H)
            ctx.interval_tally(labels, seg['path'], seg['emissions'], seg_wo, ivo, ivb, cfg.radius * STEP, req.device_hop, seg['tally'], H)
    except _lib.F2Error as e:
        if e.code == _lib.F2_ERR_NONPOSITIVE:
            raise ValueError("values must all be positive")
        raise
    out, pos = [], 0
    for b, nb in enumerate(nbs):
        rows = slice(pos, pos + nb)
        one = _Evaluated(scores[rows], labels[rows], None if levels is None else levels[b], None if track is None else track[b],
                         None, None, None)
        if occ is not None:
            one = one._replace(occlusion=dict(patches=occ['patches'], fill=occ['fill'], scores=occ['scores'][rows],
                                              summary=occ['summary'][b], map=occ['map'][b], levels=occ['levels'][b]))
        if sal is not None:
            one = one._replace(saliency=dict(bands=sal['bands'], summary=sal['summary'][b], map=sal['map'][b], levels=sal['levels'][b]))
        if seg is not None:
            ro = seg['run_offsets']
            one = one._replace(segments=dict(
                path=seg['path'][rows], emissions=seg['emissions'][rows], runs=seg['runs'][ro[b]:ro[b + 1]], value=seg['value'][b],
                tally=seg['tally'][ivo[b]:ivo[b + 1]], intervals=ivb[ivo[b]:ivo[b + 1]], logit_scale=seg_scale, penalty=seg_penalty,
                hop=req.device_hop))
        out.append(one)
        pos += nb
    return out


def EvaluateWavArrays(wavArrays, framerate, model='last_trained_model', LPF=False, CUTOFF=100,
                      FILTERBANK_COEFFICIENTS=None, ctx=None, hop=None, figure_width=None, occlusion=None,
                      occlusion_width=None, saliency=None, saliency_width=None, segments=None):
    """EvaluateOneWavArray for a list of utterances of one sample type in one device pass (f2_eval_batch): the
    filterbank and envelope kernels see the whole batch, windows and CNN run utterance by utterance. With a hop
    (f2_eval_batch_strided) every hop-th window, and the window stage and the CNN see the batch as well.
    Returns a list of (scores (nb,2) float32, labels (nb,) uint8). With figure_width=W the pass is f2_eval_figure_batch
    (hop=None: hop 1, the same rows) and every entry also holds the picture's levels (C, W) uint8 and the track (W, 5) float64
    of the decisions over the whole utterance.
    With occlusion= (True, (band, stride) or a dict: _occlusion_spec) the pass is f2_eval_occlusion_batch (hop=None: hop 1):
    scores and labels are its level 0, the same bits, and every entry ends in a dict - patches (K, 4), fill, scores (nb, K + 1, 2),
    summary (K, 4), map (K, W, 4) and levels (C, W), W = occlusion_width (default: figure_width, else FIGURE_WIDTH). With
    figure_width as well the track is f2_score_track of the level-0 scores and the levels are the occlusion call's.
    With saliency= (True, or the channels per line of the table: _saliency_bands) the pass is f2_eval_saliency_batch (hop=None: hop
    1): scores and labels are those without it, the same bits, and every entry ends in a dict - bands, summary (C, 3), map
    (C, W, 3) and levels (C, W), W = saliency_width (default: figure_width, else FIGURE_WIDTH); with figure_width as well the track
    is f2_score_track of the scores. One map per pass: not together with occlusion=.
    With segments= (True, or a dict: dwell_ms, weight, intervals - one (k, 2) array of sample intervals or None per utterance) the
    decisions are smoothed by the two-state decoder (hop=None: hop 1) and every entry ends in a dict - path, emissions, runs (n, 4),
    value, tally (k, 4), intervals, logit_scale, penalty, hop. Alone the pass is f2_eval_segments_batch; together with a figure or
    a map it is f2_decision_path, f2_decision_runs and f2_interval_tally on the scores that pass returns. Scores and labels are
    those without it, the same bits."""
    req = _Request.of(hop, figure_width, saliency_width if occlusion is None else occlusion_width, occlusion, saliency, segments)
    return [(e.scores, e.labels) + (() if e.levels is None else (e.levels, e.track))
            + tuple(d for d in (e.occlusion, e.saliency, e.segments) if d is not None)
            for e in _evaluate_arrays(wavArrays, framerate, req, model, LPF, CUTOFF, FILTERBANK_COEFFICIENTS, ctx)]


def _evaluate_group(files, loaded, req, model, LPF, CUTOFF, coefs, verbose=False):
    """The files of a group - loaded: their (source rate, rate, samples) - evaluated for `req`: (an _Evaluated per file, the names
    of its phonemes per file - None unless segments are asked for and its .PHN gives some). Files of one rate and one sample type
    are one batch pass with `coefs`, the filterbank of the configured rate (None: designed for the files' rate); mixed files go
    one at a time, with `coefs` where the rate is the configured one. A file on its own goes through the batch pass, silently, where
    req.needs_pass and through EvaluateOneWavArray, with the reference's prints, where not; `verbose` (cnn eval, evalnoise) sends
    every file without options that way."""
    rates = [fr for _, fr, _ in loaded]
    waves = [w for _, _, w in loaded]
    phonemes = [None] * len(files)
    if req.segments is not None:
        phonemes = [_file_phonemes(file, source, fr) for file, (source, fr, _) in zip(files, loaded)]
    names = [None if p is None else p[0] for p in phonemes]

    def batch_pass(members, c):
        mine = req
        if req.segments is not None:
            mine = req._replace(segments=dict(req.segments, intervals=[None if phonemes[i] is None else phonemes[i][1] for i in members]))
        return _evaluate_arrays([waves[i] for i in members], rates[members[0]], mine, model, LPF, CUTOFF, c)

    uniform = len(set(rates)) == 1 and len({numpy.asarray(w).dtype for w in waves}) == 1
    if uniform and (req.needs_pass or not verbose):
        return batch_pass(list(range(len(files))), coefs), names
    configured = F2Config().framerate
    out = []
    for i, (file, fr, w) in enumerate(zip(files, rates, waves)):
        c = coefs if uniform or fr == configured else None
        if req.needs_pass:
            out += batch_pass([i], c)
        else:
            out.append(_Evaluated(*EvaluateOneWavArray(w, fr, file, model=model, LPF=LPF, CUTOFF=CUTOFF, FILTERBANK_COEFFICIENTS=c,
                                                       hop=req.hop), None, None, None, None, None))
    return out, names


def _finish_file(one, file, stem, what, out, N, framerate, source, req, accuracy, resample, keys, names):
    """The end of a file in cnn eval / evalnoise / evalrand: figure, occlusion map, saliency map, the smoothed decisions' accuracy and
    the segment tables of its _Evaluated `one`, each where `req` asks for it, then `out`, the .F2CNN.npz. file: whose .FB / .PHN label
    it (evalnoise: the clean file); stem: of the pictures; what: its name in the segment tables; keys: what the .npz holds already -
    the accuracy keys, in cnn eval / evalnoise the rate keys too, which then stay in front. Returns every key the .npz gained."""
    keys = dict(keys)
    if req.figure_width is not None:
        keys.update(_write_figure(file, stem, one.levels, one.track, N, framerate, source, keys))
    if one.occlusion is not None:
        keys.update(_write_occlusion(file, stem, one.occlusion, N, framerate, source))
    if one.saliency is not None:
        keys.update(_write_saliency(file, stem, one.saliency, N, framerate, source))
    if one.segments is not None:
        keys.update(_smoothed_accuracy(file, one.segments, accuracy, framerate, source))
        keys.update(_write_segments(what, one.segments, framerate, names))
    keys.update(_rate_keys(resample, framerate, source))
    _save(out, one.scores, one.labels, req.hop, N, framerate, keys)
    return keys


def EvaluateOneWavFile(file, LPF=False, CUTOFF=50, model='last_trained_model', CENTER_FREQUENCIES=None,
                       FILTERBANK_COEFFICIENTS=None, hop=None, accuracy=None, resample=False, figure=False,
                       figure_width=FIGURE_WIDTH, occlusion=None, saliency=None, segments=None):
    """`cnn eval --file X.WAV`: evaluates the file, writes <base>.F2CNN.npz - scores and labels, and what the options of the
    module's docstring add - and returns (scores, labels)."""
    print('Using model', model if not isinstance(model, F2CNNModel) else '<in-memory model>')
    print("File:\t\t{}".format(file))
    source, framerate, wavArray = _load([file], resample)[0]
    req = _Request.of_command(hop, figure, figure_width, occlusion, saliency, segments)
    (one,), (names,) = _evaluate_group([file], [(source, framerate, wavArray)], req, model, LPF, CUTOFF, FILTERBANK_COEFFICIENTS,
                                       verbose=True)
    out = os.path.splitext(file)[0] + '.F2CNN.npz'
    keys = _scored_extra(file, one.labels, accuracy, hop, framerate, source, resample)
    _finish_file(one, file, os.path.splitext(os.path.basename(file))[0], file, out, len(wavArray), framerate, source, req, accuracy,
                 resample, keys, names)
    rising = int(one.labels.sum())
    print("\t\t{}\tdone ! {} windows: {} rising, {} falling -> {}".format(file, len(one.labels), rising,
                                                                          len(one.labels) - rising, out))
    return one.scores, one.labels


def EvaluateRandom(count=None, LPF=False, CUTOFF=50, model='last_trained_model', hop=None, accuracy=None, resample=False,
                   figure=False, figure_width=FIGURE_WIDTH, occlusion=None, saliency=None, segments=None):
    """`cnn evalrand`: evaluate the WAV files under resources/f2cnn/*/ in random order (all of them, or `count`
    drawn with replacement like numpy.random.choice in the reference). The filterbank is designed once and the model
    is uploaded once (the reference reloads the Keras model for every file). Files go to the device in groups of 16, a group of
    one rate and one sample type in one pass (_evaluate_group); every file gets what EvaluateOneWavFile writes and prints for it
    under the options of the module's docstring. With accuracy= a group is scored in one device pass per rate and the corpus total
    is printed from the summed confusion matrices; with occlusion= / saliency= the table of the corpus is printed at the end,
    counts summed and means weighted by rows (CombineOcclusionSummaries, CombineSaliencySummaries)."""
    import glob
    import time
    TotalTime = time.time()
    wavFiles = sorted(glob.glob(os.path.join('resources', 'f2cnn', '*', '*.WAV')))
    if not wavFiles:
        print("NO WAV FILES FOUND")
        exit(-1)
    print("\n###############################\nEvaluating network on {} WAV files in '{}'.".format(
        len(wavFiles), os.path.split(wavFiles[0])[0]))
    cfg = F2Config()
    CENTER_FREQUENCIES = filters.centre_freqs(cfg.framerate, cfg.nchannels, cfg.low_freq)
    FILTERBANK_COEFFICIENTS = filters.make_erb_filters(cfg.framerate, CENTER_FREQUENCIES)
    if not isinstance(model, F2CNNModel):
        model = load_model(model)
    if count is None:
        wavFiles = list(numpy.random.permutation(wavFiles))
    elif count > 1:
        wavFiles = list(numpy.random.choice(wavFiles, count))
    results = {}
    if accuracy is not None:
        _accuracy_origin(accuracy, 0, 0)
        corpus = numpy.zeros((2, 2), numpy.int64)
    occlusion_corpus = []                         # (patches, hz, summary) per file
    saliency_corpus = []                          # (framerate, summary) per file
    BATCH = 16                                    # files per device pass
    req = _Request.of_command(hop, figure, figure_width, occlusion, saliency, segments)
    for s0 in range(0, len(wavFiles), BATCH):
        group = wavFiles[s0:s0 + BATCH]
        loaded = _load(group, resample)
        outs, phoneme_names = _evaluate_group(group, loaded, req, model, LPF, CUTOFF, FILTERBANK_COEFFICIENTS)
        extras = [{} for _ in group]
        if accuracy is not None:
            refs = [ReferenceLabels(file) if source == fr else None for file, (source, fr, _) in zip(group, loaded)]
            for file, ref, (source, fr, _) in zip(group, refs, loaded):
                if source != fr:
                    _no_rate_accuracy(file, source, fr)
                elif ref is None:
                    _no_side_files(file)
            # one pass per framerate of the group (the step is in samples of the file)
            for rate in sorted({fr for (_, fr, _), ref in zip(loaded, refs) if ref is not None}):
                members = [i for i, ((_, fr, _), ref) in enumerate(zip(loaded, refs)) if fr == rate and ref is not None]
                wo = numpy.concatenate([[0], numpy.cumsum([len(outs[i].labels) for i in members])]).astype(numpy.int64)
                confusions = _confusions(_lib.default_context(), numpy.concatenate([outs[i].labels for i in members]), wo,
                                         [refs[i] for i in members], accuracy, hop, _step(rate, cfg))
                for i, confusion in zip(members, confusions):
                    _print_accuracy(group[i], confusion, accuracy)
                    extras[i] = _accuracy_keys(confusion, accuracy)
                    corpus += confusion
        for file, (source, fr, w), one, extra, names in zip(group, loaded, outs, extras, phoneme_names):
            out = os.path.splitext(file)[0] + '.F2CNN.npz'
            keys = _finish_file(one, file, os.path.splitext(os.path.basename(file))[0], file, out, len(w), fr, source, req, accuracy,
                                resample, extra, names)
            if occlusion is not None:
                if occlusion_corpus and not numpy.array_equal(occlusion_corpus[0][0], keys['occlusion_patches']):
                    occlusion_corpus = None       # (files of another channel count: no common table)
                if occlusion_corpus is not None:
                    occlusion_corpus.append((keys['occlusion_patches'], keys['occlusion_hz'], keys['occlusion_summary']))
            if saliency is not None:
                saliency_corpus.append((fr, keys['saliency_summary']))
            rising = int(one.labels.sum())
            print("\t\t{}\tdone ! {} windows: {} rising, {} falling -> {}".format(file, len(one.labels), rising,
                                                                                  len(one.labels) - rising, out))
            results[file] = (one.scores, one.labels)
    print("Evaluating network on all files.")
    if accuracy is not None:
        _print_accuracy("all files", corpus, accuracy)
    if occlusion is not None and occlusion_corpus:
        for line in OcclusionTable("all files", occlusion_corpus[0][0], occlusion_corpus[0][1],
                                   CombineOcclusionSummaries([summary for _, _, summary in occlusion_corpus])):
            print(line)
    if saliency is not None and saliency_corpus and len({(fr, len(summary)) for fr, summary in saliency_corpus}) == 1:
        cf = numpy.asarray(filters.centre_freqs(saliency_corpus[0][0], len(saliency_corpus[0][1]), cfg.low_freq), numpy.float64)
        for line in SaliencyTable("all files", cf, CombineSaliencySummaries([summary for _, summary in saliency_corpus]), req.saliency):
            print(line)
    print('              Total time:', time.time() - TotalTime)
    print('')
    return results


def SNRdbToSNRlinear(SNRdb):
    return 10 ** (SNRdb / 10.0)


def RMS(signal):
    """Root mean square of a signal (computed in float64: int16 squares would overflow)."""
    return numpy.sqrt(numpy.mean(numpy.square(numpy.asarray(signal, dtype=numpy.float64))))


def _noisy_copy_paths(file, SNRdB):
    """Where `cnn evalnoise` puts its outputs (reference layout, Evaluating.py:203-206): OutputWavFiles/addedNoise/<stem><SNR>dB.*"""
    stem = os.path.basename(os.path.splitext(file)[0])
    target = os.path.join('OutputWavFiles', 'addedNoise', '{}{}dB'.format(stem, SNRdB))
    return os.path.splitext(file)[0], target


def add_gaussian_noise(wave, SNRdB, rng=None):
    """wave + N(0, sigma^2), sigma = RMS(wave) / 10^(SNRdB / 10) - the reference's scaling (Evaluating.py:199), which divides
    by the POWER ratio where an amplitude ratio would be 10^(SNRdB / 20); reproduced, not corrected. float64 out."""
    sigma = RMS(wave) / SNRdbToSNRlinear(SNRdB)
    draw = (rng or numpy.random).normal
    return numpy.asarray(wave, dtype=numpy.float64) + draw(scale=sigma, size=len(wave))


def EvaluateWithNoise(file, LPF=False, CUTOFF=100, model='last_trained_model', CENTER_FREQUENCIES=None,
                      FILTERBANK_COEFFICIENTS=None, SNRdB=-3, rng=None, hop=None, accuracy=None, resample=False, figure=False,
                      figure_width=FIGURE_WIDTH, occlusion=None, saliency=None, segments=None):
    """`cnn evalnoise` (reference: scripts/CNN/Evaluating.py:193-221): the file plus Gaussian noise at the requested level is
    written next to copies of its annotation files under OutputWavFiles/addedNoise/ and the float64 waveform is evaluated by
    the device pipeline. Returns (scores, labels) and also leaves them in <target>.F2CNN.npz; `rng` (a numpy Generator or
    RandomState) makes the noise reproducible - the reference draws from the global numpy state. With resample= the noise is
    added to the resampled, one-channel signal and the noisy WAV is written at the configured framerate. The options of the
    module's docstring apply to the noisy run: pictures and tables carry the noisy file's name, and labels, formant, slope and
    phonemes are those of the clean file's .FB / .PHN (what the copies under addedNoise/ are there for)."""
    import shutil
    from scipy.io import wavfile
    print("File:\t\t{}".format(file))
    print("Appyling gaussian noise, new SNR is {SNR}dB".format(SNR=SNRdB))      # (the reference's wording, kept for log parsers)
    source_rate, framerate, clean = _load([file], resample)[0]
    noisy = add_gaussian_noise(clean, SNRdB, rng)
    source, target = _noisy_copy_paths(file, SNRdB)
    os.makedirs(os.path.dirname(target), exist_ok=True)
    wavfile.write(target + '.WAV', framerate, noisy)
    # annotation files travel with the audio where they exist (the reference gives up on all three at the first missing one)
    for ext in ('.FB', '.PHN', '.WRD'):
        if os.path.exists(source + ext):
            shutil.copyfile(source + ext, target + ext)
    print('New noisy WAVE file saved as', target + '.WAV')
    req = _Request.of_command(hop, figure, figure_width, occlusion, saliency, segments)
    (one,), (names,) = _evaluate_group([file], [(source_rate, framerate, noisy)], req, model, LPF, CUTOFF, FILTERBANK_COEFFICIENTS,
                                       verbose=True)
    keys = _scored_extra(file, one.labels, accuracy, hop, framerate, source_rate, resample)
    _finish_file(one, file, os.path.basename(target), target + '.WAV', target + '.F2CNN.npz', len(noisy), framerate, source_rate, req,
                 accuracy, resample, keys, names)
    print("\t\t{}\tdone !".format(file))
    return one.scores, one.labels


# ---- the robustness sweeps: a file at K levels of one axis (noise, envelope cutoff, room) and at the unchanged level, the
# referee, in one device pass per group of files. _run_sweep is the file driver; an axis says what is its own ----------------
def _level_text(value):
    """how a level is printed and named: 10.0 -> '10', -3.0 -> '-3', 2.5 -> '2.5'"""
    return '{:g}'.format(float(value))


LEVELS_LIMIT = 8 << 30           # bytes of envelope levels one device pass of EvaluateCutoffSweep may ask for


def _cutoff_groups(members, K, Cn, batch=16, limit=LEVELS_LIMIT):
    """members [(file, wave)] in passes of up to `batch` files whose (K + 1) * Cn * samples * 8 bytes of levels stay within
    `limit` (a single file beyond it still gets a pass of its own)"""
    group, samples = [], 0
    for file, wave in members:
        n = wave.shape[0]
        if group and (len(group) == batch or (K + 1) * Cn * (samples + n) * 8 > limit):
            yield group
            group, samples = [], 0
        group.append((file, wave))
        samples += n
    if group:
        yield group


class _SweepAxis(collections.namedtuple('_SweepAxis', 'names referee label limit call own order out outdir wav_target')):
    """What a sweep has of its own. names: how its K levels are printed; referee: the key and printed name of level K ('clean');
    label: the format of a name at the start of a level's line. limit: bytes of levels a pass may ask for (_cutoff_groups).
    call(ctx, handle, flat, dt, offsets, coefs, B, Cn, radius, STEP, hop, framerate, labels) -> (window offsets, stats, the
    level waveforms or None, whatever own needs); own(got, rows, wo, n, radius, STEP, hop, framerate) -> the axis's keys of a
    file of n samples whose levels are utterances `rows`: those `order` names go into the .npz in that order among windows ...
    hop, the others behind the labels. out(file): the .npz; outdir: made before the first .npz of a pass (None: the file's own);
    wav_target(file, l): the path, without extension, of level l's WAV and side-file copies (None: no WAVs)."""


def _run_sweep(axis, files, hop, model, ctx, accuracy, resample):
    K = len(axis.names)
    hop = 1 if hop is None else int(hop)
    if accuracy is not None:
        _accuracy_origin(accuracy, 0, 0)
    ctx = ctx or _lib.default_context()
    cfg = F2Config()
    if not isinstance(model, F2CNNModel):
        model = load_model(model)
    read = _load(files, resample)
    sources = {file: source for file, (source, _, _) in zip(files, read)}
    groups = {}                                   # one framerate and sample type per call
    for file, (_, framerate, wavArray) in zip(files, read):
        wave, dt = filters._wave_args(wavArray)
        groups.setdefault((framerate, dt), []).append((file, wave))
    keys = [str(k) for k in range(K)] + [axis.referee]          # labels_<k>: level k
    names = list(axis.names) + [axis.referee]
    line = "\t" + axis.label + "\t{} windows\t{} rising\tagreement with " + axis.referee + " {:.4f}"
    results = {}
    for (framerate, dt), members in groups.items():
        coefs = numpy.ascontiguousarray(filters.make_erb_filters(framerate, filters.centre_freqs(framerate, cfg.nchannels,
                                                                                                  cfg.low_freq)))
        Cn = coefs.shape[0]
        STEP = _step(framerate, cfg)
        for group in _cutoff_groups(members, K, Cn, limit=axis.limit):
            B = len(group)
            offsets = numpy.zeros(B + 1, numpy.int64)
            offsets[1:] = numpy.cumsum([w.shape[0] for _, w in group])
            flat = numpy.concatenate([w for _, w in group])
            nbh = [_lib.strided_window_count(w.shape[0], cfg.radius, STEP, hop) for _, w in group]
            labels = numpy.empty((K + 1) * sum(nbh), numpy.uint8)
            try:
                wo, stats, waves, got = axis.call(ctx, model.handle(ctx), flat, dt, offsets, coefs, B, Cn, cfg.radius, STEP, hop,
                                                  framerate, labels)
            except _lib.F2Error as e:
                if e.code == _lib.F2_ERR_NONPOSITIVE:
                    raise ValueError("values must all be positive")
                raise
            assert list(numpy.diff(wo)) == nbh * (K + 1)
            refs = [None] * B
            if accuracy is not None:     # (the labels of a file whose rate differed count source samples)
                refs = [ReferenceLabels(file) if sources[file] == framerate else None for file, _ in group]
            confusions = None
            if any(ref is not None for ref in refs):
                confusions = _confusions(ctx, labels, wo, refs, accuracy, hop, STEP)
            if axis.outdir:
                os.makedirs(axis.outdir, exist_ok=True)
            for b, (file, w) in enumerate(group):
                rows = [l * B + b for l in range(K + 1)]
                windows = numpy.array([wo[u + 1] - wo[u] for u in rows], numpy.int64)
                rising, agree = stats[rows, 0].copy(), stats[rows, 1].copy()
                with numpy.errstate(invalid='ignore', divide='ignore'):
                    agreement = numpy.where(windows > 0, agree / windows.astype(numpy.float64), numpy.nan)
                own = dict(axis.own(got, rows, wo, w.shape[0], cfg.radius, STEP, hop, framerate), windows=windows, rising=rising,
                           agree=agree, agreement=agreement, hop=numpy.int64(hop))
                res = dict({key: own.pop(key) for key in axis.order}, **_rate_keys(resample, framerate, sources[file]))
                for key, u in zip(keys, rows):
                    res['labels_' + key] = labels[wo[u]:wo[u + 1]].copy()
                res.update(own)
                if refs[b] is not None:
                    res['confusion'] = confusions[rows].copy()
                    res['accuracy_vtr'] = _accuracy_of(res['confusion'])
                out = axis.out(file)
                numpy.savez(out, **res)
                print("File:\t\t{}".format(file))
                if accuracy is not None and sources[file] != framerate:
                    _no_rate_accuracy(file, sources[file], framerate)
                elif accuracy is not None and refs[b] is None:
                    _no_side_files(file)
                for l in range(K + 1):
                    text = line.format(names[l], windows[l], rising[l], agreement[l])
                    if refs[b] is not None:
                        text += "\taccuracy against the VTR labels ({}) {:.4f}".format(accuracy, res['accuracy_vtr'][l])
                    print(text)
                if waves is not None:
                    import shutil
                    from scipy.io import wavfile
                    source = os.path.splitext(file)[0]
                    for l in range(K):
                        target = axis.wav_target(file, l)
                        lo = l * int(offsets[-1]) + int(offsets[b])
                        wavfile.write(target + '.WAV', framerate, waves[lo:lo + w.shape[0]])
                        for ext in ('.FB', '.PHN', '.WRD'):
                            if os.path.exists(source + ext):
                                shutil.copyfile(source + ext, target + ext)
                print("\t\t{}\tdone ! -> {}".format(file, out))
                results[file] = res
    return results


def EvaluateNoiseSweep(files, SNRdBs, seed=0, hop=None, LPF=False, CUTOFF=50, model='last_trained_model', save_wavs=False,
                       ctx=None, accuracy=None, resample=False, maskers=None, colours=None, noise_taps=1025):
    """`cnn noisesweep` (not in the reference, whose EvaluateWithNoise :193-221 takes one file at one level): every file at
    every level of SNRdBs and clean in one device pass per group of files (f2_eval_noise_sweep: the noise is drawn on the device
    from (seed, level, file's place in its group, sample), so a sweep repeats bit for bit), with the clean run of the same
    network as the referee. Per file, OutputWavFiles/addedNoise/<stem>.sweep.npz holds snr_db, sigma, windows, rising, agree,
    agreement (= agree / windows, NaN without windows) - one entry per level, the clean level last - seed, hop and labels_<k>
    for level k of snr_db (labels_clean for the clean one); one line per level is printed and the same data is returned as a dict per
    file. save_wavs also writes <stem><SNR>dB.WAV with copies of the annotation files, as EvaluateWithNoise names and writes
    them. Files are grouped like EvaluateRandom groups them: one framerate and sample type per call, 16 files per pass. hop=None
    is hop 1.
    With accuracy= every level of a file that has its .FB / .PHN is also scored against their labels (one f2_label_accuracy
    call per group): the file's results gain accuracy_vtr (K+1) and confusion (K+1, 2, 2), [level][ref][pred], the clean level
    last, and the printed lines the accuracy. With resample= the files are brought to the configured framerate first (one
    device call per kind of file), the results gain framerate and source_framerate, and a file whose rate differed is left out
    of the accuracy.
    With colours= (`--colours`: names of noise.COLOURS, 'like:<recording.wav>', 'fir:<taps.npy>') the noise of a level is
    Gaussian noise of that colour (f2_eval_shaped_noise_sweep: the same deviates through a filter of noise_taps taps, built once
    per framerate by noise.FromSpec and normalised to sum h^2 = 1, so an SNR means what it means without the option). The levels
    are colour-major over SNRdBs, at most 64, named like 'pink 10dB'; the file is <stem>.coloursweep.npz - a white sweep's
    .sweep.npz is never overwritten - with the keys above, snr_db per level, and colours (a string per level), fir and fir_offsets
    (the taps of all levels and where each level's start); save_wavs writes <stem>_<colour>_<SNR>dB.WAV. colours=None is the
    white sweep as it was, to the byte.
    With maskers= (`--maskers`: recordings, read by masker.LoadMasker at the files' framerate, with resample= at any rate) a level
    is a recording at an SNR and nothing is Gaussian: per file a cyclic segment of the recording, drawn from (seed, recording,
    file's place in its group), is scaled to sigma and mixed in (f2_eval_masker_sweep). The levels are masker-major over SNRdBs
    (masker.MaskerLevels), at most 64, named like 'babble 10dB'; the file is <stem>.maskersweep.npz with snr_db, maskers (a
    name per level), masker_files, sigma, gain and start per level, then the keys above; save_wavs writes
    <stem>_<masker>_<SNR>dB.WAV. Not together with colours=."""
    if isinstance(files, (str, bytes, os.PathLike)):
        files = [files]
    snr = numpy.asarray(SNRdBs, dtype=numpy.float64).reshape(-1)
    if not len(snr) or not numpy.isfinite(snr).all():
        raise ValueError("a noise sweep needs at least one finite SNR in dB")
    if maskers is not None:
        if colours is not None:
            raise ValueError("a noise sweep has colours or maskers, not both")
        return _EvaluateMaskerSweep(files, snr, maskers, seed, hop, LPF, CUTOFF, model, save_wavs, ctx, accuracy, resample)
    if colours is not None:
        return _EvaluateColourSweep(files, snr, colours, noise_taps, seed, hop, LPF, CUTOFF, model, save_wavs, ctx, accuracy, resample)
    K = len(snr)

    def call(ctx, handle, flat, dt, offsets, coefs, B, Cn, radius, STEP, hop, framerate, labels):
        noisy = numpy.empty((K + 1) * int(offsets[-1]), numpy.float64) if save_wavs else None
        wo, sigma, stats = ctx.eval_noise_sweep(handle, flat, dt, offsets, coefs, B, Cn, bool(LPF), CUTOFF if LPF else 0.0,
                                                FFT_PRECISION, radius, STEP, hop, snr, seed, noisy, None, labels, _lib.MEM_HOST)
        return wo, stats, noisy, sigma

    def own(sigma, rows, wo, n, radius, STEP, hop, framerate):
        return dict(snr_db=snr.copy(), sigma=sigma[rows].copy(), seed=numpy.uint64(int(seed) & (2 ** 64 - 1)))

    outdir = os.path.join('OutputWavFiles', 'addedNoise')
    axis = _SweepAxis(names=[_level_text(v) + 'dB' for v in snr], referee='clean', label="SNR {:>8}", limit=float('inf'), call=call,
                      own=own, order=('snr_db', 'sigma', 'windows', 'rising', 'agree', 'agreement', 'seed', 'hop'),
                      out=lambda file: os.path.join(outdir, os.path.basename(_noisy_copy_paths(file, 0)[0]) + '.sweep.npz'),
                      outdir=outdir, wav_target=lambda file, l: _noisy_copy_paths(file, snr[l])[1])
    return _run_sweep(axis, files, hop, model, ctx, accuracy, resample)


COLOUR_LEVELS_MAX = 64


def ColourLevels(colours, snrs):
    """The level grid of a coloured sweep, colour-major over the SNRs: [(colour spec, printed colour, SNR)] - level
    c * len(snrs) + s is colour c at SNR s. ValueError for no colour, an unknown one, or more than COLOUR_LEVELS_MAX levels."""
    from ... import noise
    if isinstance(colours, str):
        colours = colours.split(',')
    colours = [str(c) for c in colours]
    if not colours or not all(colours):
        raise ValueError("a coloured noise sweep needs at least one colour")
    for c in colours:
        if not c.startswith(('like:', 'fir:')) and c not in noise.COLOURS:
            raise ValueError("unknown noise colour {!r} (one of {}, like:<recording.wav>, fir:<taps.npy>)".format(
                c, ', '.join(noise.COLOURS)))
        if c in ('like:', 'fir:'):
            raise ValueError("{} needs a file name behind it".format(c))
    if len(colours) * len(snrs) > COLOUR_LEVELS_MAX:
        raise ValueError("a noise sweep takes at most {} levels, not {} colours x {} SNRs = {}".format(
            COLOUR_LEVELS_MAX, len(colours), len(snrs), len(colours) * len(snrs)))
    return [(c, noise.SpecName(c), float(v)) for c in colours for v in snrs]


def _EvaluateColourSweep(files, snr, colours, noise_taps, seed, hop, LPF, CUTOFF, model, save_wavs, ctx, accuracy, resample):
    """EvaluateNoiseSweep with colours: the arguments are checked before any file is read"""
    from ... import noise
    grid = ColourLevels(colours, snr)
    noise._check_taps(noise_taps)
    K = len(grid)
    level_snr = numpy.array([v for _, _, v in grid], numpy.float64)
    level_colour = numpy.array([name for _, name, _ in grid], dtype=str)
    filters_at = {}                               # per framerate: one filter per colour, shared by its levels

    def firs(framerate):
        if framerate not in filters_at:
            built = {}
            for spec, _, _ in grid:
                if spec not in built:
                    built[spec] = noise.FromSpec(spec, framerate, noise_taps)
            filters_at[framerate] = [built[spec] for spec, _, _ in grid]
        return filters_at[framerate]

    def call(ctx, handle, flat, dt, offsets, coefs, B, Cn, radius, STEP, hop, framerate, labels):
        noisy = numpy.empty((K + 1) * int(offsets[-1]), numpy.float64) if save_wavs else None
        wo, sigma, stats = ctx.eval_shaped_noise_sweep(handle, flat, dt, offsets, coefs, B, Cn, bool(LPF), CUTOFF if LPF else 0.0,
                                                       FFT_PRECISION, radius, STEP, hop, level_snr, firs(framerate), seed, noisy, None,
                                                       labels, _lib.MEM_HOST)
        return wo, stats, noisy, sigma

    def own(sigma, rows, wo, n, radius, STEP, hop, framerate):
        hs = firs(framerate)
        return dict(snr_db=level_snr.copy(), colours=level_colour.copy(), sigma=sigma[rows].copy(),
                    seed=numpy.uint64(int(seed) & (2 ** 64 - 1)), fir=numpy.concatenate(hs),
                    fir_offsets=numpy.concatenate([[0], numpy.cumsum([len(h) for h in hs])]).astype(numpy.int64))

    outdir = os.path.join('OutputWavFiles', 'addedNoise')
    stem = lambda file: os.path.basename(os.path.splitext(file)[0])
    axis = _SweepAxis(names=['{} {}dB'.format(name, _level_text(v)) for _, name, v in grid], referee='clean', label="{:>16}",
                      limit=float('inf'), call=call, own=own,
                      order=('snr_db', 'colours', 'sigma', 'windows', 'rising', 'agree', 'agreement', 'seed', 'hop'),
                      out=lambda file: os.path.join(outdir, stem(file) + '.coloursweep.npz'), outdir=outdir,
                      wav_target=lambda file, l: os.path.join(outdir, '{}_{}_{}dB'.format(stem(file), grid[l][1], _level_text(grid[l][2]))))
    return _run_sweep(axis, files, hop, model, ctx, accuracy, resample)


def _EvaluateMaskerSweep(files, snr, maskers, seed, hop, LPF, CUTOFF, model, save_wavs, ctx, accuracy, resample):
    """EvaluateNoiseSweep with maskers: the grid is checked before any file is read, a recording is read once per framerate"""
    from ... import masker
    if isinstance(maskers, str):
        maskers = maskers.split(',')
    maskers = [str(m) for m in maskers]
    grid = masker.MaskerLevels(maskers, snr)
    K = len(grid)
    level_snr = numpy.array([v for _, _, v in grid], numpy.float64)
    level_name = numpy.array([name for _, name, _ in grid], dtype=str)
    masker_of = numpy.array([r for r, _, _ in grid], numpy.int32)
    recordings_at = {}

    def recordings(framerate):
        if framerate not in recordings_at:
            recordings_at[framerate] = [masker.LoadMasker(m, framerate, resample=bool(resample)) for m in maskers]
        return recordings_at[framerate]

    def call(ctx, handle, flat, dt, offsets, coefs, B, Cn, radius, STEP, hop, framerate, labels):
        noisy = numpy.empty((K + 1) * int(offsets[-1]), numpy.float64) if save_wavs else None
        wo, sigma, stats, gain, start = ctx.eval_masker_sweep(handle, flat, dt, offsets, coefs, B, Cn, bool(LPF), CUTOFF if LPF else 0.0,
                                                              FFT_PRECISION, radius, STEP, hop, level_snr, recordings(framerate), masker_of,
                                                              seed, noisy, None, labels, _lib.MEM_HOST)
        return wo, stats, noisy, (sigma, gain, start)

    def own(got, rows, wo, n, radius, STEP, hop, framerate):
        sigma, gain, start = got
        return dict(snr_db=level_snr.copy(), maskers=level_name.copy(), masker_files=numpy.array(maskers, dtype=str), sigma=sigma[rows].copy(),
                    gain=gain[rows].copy(), start=start[rows].copy(), seed=numpy.uint64(int(seed) & (2 ** 64 - 1)))

    outdir = os.path.join('OutputWavFiles', 'addedNoise')
    stem = lambda file: os.path.basename(os.path.splitext(file)[0])
    axis = _SweepAxis(names=['{} {}dB'.format(name, _level_text(v)) for _, name, v in grid], referee='clean', label="{:>16}",
                      limit=float('inf'), call=call, own=own,
                      order=('snr_db', 'maskers', 'masker_files', 'sigma', 'gain', 'start', 'windows', 'rising', 'agree', 'agreement', 'seed',
                             'hop'),
                      out=lambda file: os.path.join(outdir, stem(file) + '.maskersweep.npz'), outdir=outdir,
                      wav_target=lambda file, l: os.path.join(outdir, '{}_{}_{}dB'.format(stem(file), grid[l][1], _level_text(grid[l][2]))))
    return _run_sweep(axis, files, hop, model, ctx, accuracy, resample)


# ---- `cnn lpfsweep`: one file at several envelope cutoffs (the modulation axis; not in the reference, whose route is one
# `cnn eval --lpf HZ` per cutoff) ---------------------------------------------------------------------------------------------
def EvaluateCutoffSweep(files, cutoffs, hop=None, model='last_trained_model', ctx=None, accuracy=None, resample=False):
    """`cnn lpfsweep`: every file at every envelope cutoff of `cutoffs` (Hz) and unfiltered in one device pass per group of
    files (f2_eval_cutoff_sweep: filterbank and Hilbert envelope run once, the first-order low-pass of EnvelopeExtraction.py:39-67
    K times on the result, in float64), with the unfiltered run of the same network as the referee. Per file, <base>.lpfsweep.npz
    next to the WAV holds cutoff_hz, windows, rising, agree, agreement (= agree / windows, NaN without windows) - K + 1 entries
    each, the unfiltered level last - hop, timepoints, scores (K + 1, n, 2) and labels_<k> for level k of cutoff_hz (labels_nolpf
    for the unfiltered one); one line per level is printed and the same data is returned as a dict per file. Files are grouped
    like EvaluateNoiseSweep groups them - one framerate and sample type per call, up to 16 files - and a group is cut short where
    its levels would take more than 8 GiB. hop=None is hop 1. accuracy= and resample= as in EvaluateNoiseSweep: confusion
    (K + 1, 2, 2) and accuracy_vtr (K + 1) per file that has its .FB / .PHN (one f2_label_accuracy call per group), framerate and
    source_framerate."""
    if isinstance(files, (str, bytes, os.PathLike)):
        files = [files]
    cut = numpy.asarray(cutoffs, dtype=numpy.float64).reshape(-1)
    if not len(cut) or not numpy.isfinite(cut).all() or (cut <= 0).any() or (cut >= 8000).any():
        raise ValueError("a cutoff sweep needs at least one finite cutoff in (0, 8000) Hz")

    def call(ctx, handle, flat, dt, offsets, coefs, B, Cn, radius, STEP, hop, framerate, labels):
        scores = numpy.empty((len(labels), 2), numpy.float32)
        wo, stats = ctx.eval_cutoff_sweep(handle, flat, dt, offsets, coefs, B, Cn, FFT_PRECISION, radius, STEP, hop, cut, None, scores,
                                          labels, _lib.MEM_HOST)
        return wo, stats, None, scores

    def own(scores, rows, wo, n, radius, STEP, hop, framerate):
        return dict(cutoff_hz=cut.copy(), timepoints=_lib.strided_timepoints(n, radius, STEP, hop),
                    scores=numpy.stack([scores[wo[u]:wo[u + 1]] for u in rows]))

    axis = _SweepAxis(names=[_level_text(v) + 'Hz' for v in cut], referee='nolpf', label="cutoff {:>8}", limit=LEVELS_LIMIT, call=call,
                      own=own, order=('cutoff_hz', 'windows', 'rising', 'agree', 'agreement', 'hop', 'timepoints', 'scores'),
                      out=lambda file: os.path.splitext(file)[0] + '.lpfsweep.npz', outdir=None, wav_target=None)
    return _run_sweep(axis, files, hop, model, ctx, accuracy, resample)


# ---- `cnn reverbsweep`: one file at several reverberation times (the room axis; not in the reference, whose only route is a
# host convolution, a WAV per room and one `cnn eval` per WAV) ---------------------------------------------------------------
def _reverb_copy_paths(file, name):
    """Where `cnn reverbsweep` puts its outputs: OutputWavFiles/reverb/<stem><name>.*"""
    stem = os.path.basename(os.path.splitext(file)[0])
    return os.path.splitext(file)[0], os.path.join('OutputWavFiles', 'reverb', stem + name)


def EvaluateReverbSweep(files, t60s=(), rirs=(), drr_db=0.0, seed=0, hop=None, LPF=False, CUTOFF=50, model='last_trained_model',
                        save_wavs=False, ctx=None, accuracy=None, resample=False):
    """`cnn reverbsweep`: every file convolved with every impulse response and dry in one device pass per group of files
    (f2_eval_reverb_sweep: the causal convolution truncated to the file's own length, in float64, so a level keeps the window
    count and the time axis of the dry one), with the dry run of the same network as the referee. The levels are the t60s
    (seconds) in the order given - synthetic responses, reverb.SyntheticRIR(t60, framerate, drr_db, seed, level) - then the
    measured responses of the WAV files `rirs` (reverb.LoadRIR), then `dry`; the responses are built once per framerate. Per
    file, OutputWavFiles/reverb/<stem>.reverbsweep.npz holds t60, rir_files, drr_db, seed, taps, windows, rising, agree,
    agreement (= agree / windows, NaN without windows) - windows ... agreement with one entry per level, the dry level last - hop,
    labels_<k> for level k (labels_dry for the dry one) and rir_<k>, the response level k was made with (NumPy does not promise
    standard_normal's stream across versions); one line per level is printed and the same data is returned as a dict per file.
    save_wavs also writes <stem>_T60_<value>s.WAV (or <stem>_<rir stem>.WAV) with copies of the annotation files. Files are
    grouped like EvaluateNoiseSweep groups them: one framerate and sample type per call, 16 files per pass. hop=None is hop 1.
    accuracy= and resample= as in EvaluateNoiseSweep: confusion (K+1, 2, 2) and accuracy_vtr (K+1) per file that has its .FB /
    .PHN, framerate and source_framerate. The arguments are checked before any file is read."""
    from ... import reverb
    if isinstance(files, (str, bytes, os.PathLike)):
        files = [files]
    if isinstance(rirs, (str, bytes, os.PathLike)):
        rirs = [rirs]
    t60 = numpy.asarray(t60s, dtype=numpy.float64).reshape(-1)
    rir_files = [os.fspath(r) for r in rirs]
    if not numpy.isfinite(t60).all() or (t60 <= 0).any():
        raise ValueError("a reverberation time must be finite and positive (seconds)")
    K = len(t60) + len(rir_files)
    if K < 1:
        raise ValueError("a reverberation sweep needs at least one reverberation time or impulse response file")
    if K > 64:
        raise ValueError("a reverberation sweep takes at most 64 levels, not {}".format(K))
    drr_db = float(drr_db)
    if not numpy.isfinite(drr_db):
        raise ValueError("drr_db must be finite")
    suffixes = ['_T60_' + _level_text(v) + 's' for v in t60] + ['_' + os.path.splitext(os.path.basename(r))[0] for r in rir_files]
    responses = {}                                # per framerate

    def call(ctx, handle, flat, dt, offsets, coefs, B, Cn, radius, STEP, hop, framerate, labels):
        if framerate not in responses:
            responses[framerate] = [reverb.SyntheticRIR(v, framerate, drr_db, seed, level) for level, v in enumerate(t60)] + \
                                   [reverb.LoadRIR(r, framerate) for r in rir_files]
        wet = numpy.empty((K + 1) * int(offsets[-1]), numpy.float64) if save_wavs else None
        wo, stats = ctx.eval_reverb_sweep(handle, flat, dt, offsets, coefs, B, Cn, bool(LPF), CUTOFF if LPF else 0.0, FFT_PRECISION,
                                          radius, STEP, hop, responses[framerate], wet, None, labels, _lib.MEM_HOST)
        return wo, stats, wet, None

    def own(_, rows, wo, n, radius, STEP, hop, framerate):
        hs = responses[framerate]
        return dict(t60=t60.copy(), rir_files=numpy.array(rir_files, dtype=str), drr_db=numpy.float64(drr_db), seed=numpy.int64(seed),
                    taps=numpy.array([len(h) for h in hs], numpy.int64), **{'rir_' + str(k): h.copy() for k, h in enumerate(hs)})

    axis = _SweepAxis(names=['T60 ' + _level_text(v) + 's' for v in t60] + [os.path.basename(r) for r in rir_files], referee='dry',
                      label="{:>12}", limit=float('inf'), call=call, own=own,
                      order=('t60', 'rir_files', 'drr_db', 'seed', 'taps', 'windows', 'rising', 'agree', 'agreement', 'hop'),
                      out=lambda file: _reverb_copy_paths(file, '')[1] + '.reverbsweep.npz',
                      outdir=os.path.join('OutputWavFiles', 'reverb'), wav_target=lambda file, l: _reverb_copy_paths(file, suffixes[l])[1])
    return _run_sweep(axis, files, hop, model, ctx, accuracy, resample)


# ---- `cnn smearsweep`: one file at several spectral resolutions (the twin of the modulation axis; not in the reference, and
# without the device call a host matrix product per level on envelopes that had to come down first) ---------------------------
def SmearLevels(spreads, bands, nchannels):
    """(spread (float64), counts (int64), names) of the spectral resolutions of `cnn smearsweep` and `cnn train --augment-spreads /
    --augment-bands`: the spreads in the order given, then the numbers of bands; a level's number is its place in names.
    ValueError for a spread that is not finite and positive, a number of bands that is not whole or not in 1 .. nchannels, no
    level at all, or more than 64."""
    spread = numpy.asarray(spreads, dtype=numpy.float64).reshape(-1)
    if not numpy.isfinite(spread).all() or (spread <= 0).any():
        raise ValueError("a spread must be finite and positive (ERB)")
    counts = numpy.asarray(bands).reshape(-1)
    if len(counts) and (counts != numpy.floor(counts)).any():
        raise ValueError("a number of bands must be a whole number")
    counts = counts.astype(numpy.int64)
    if (counts < 1).any() or (counts > nchannels).any():
        raise ValueError("a number of bands must lie between 1 and the {} channels".format(nchannels))
    K = len(spread) + len(counts)
    if K < 1:
        raise ValueError("a smear sweep needs at least one spread or number of bands")
    if K > 64:
        raise ValueError("a smear sweep takes at most 64 levels, not {}".format(K))
    return spread, counts, [_level_text(v) + 'ERB' for v in spread] + ['{}bands'.format(v) for v in counts]


def EvaluateSmearSweep(files, spreads=(), bands=(), hop=None, LPF=False, CUTOFF=50, model='last_trained_model', ctx=None,
                       accuracy=None, resample=False):
    """`cnn smearsweep`: every file at every spectral resolution and sharp in one device pass per group of files
    (f2_eval_smear_sweep: filterbank and envelope run once - low-passed at CUTOFF if LPF - and every level is a linear map across
    the channels of those envelopes, in float64), with the sharp run of the same network as the referee. The levels are the
    `spreads` in the order given - channel interaction, a Gaussian of that many ERB (smear.SmearMatrix on the group's centre
    frequencies) - then the `bands` - an N-band vocoder (smear.BandMatrix) - then `sharp`. Per file, <base>.smearsweep.npz next
    to the WAV holds spread_erb (K, NaN for a band level), bands (K, 0 for a spread level), windows, rising, agree, agreement
    (= agree / windows, NaN without windows) - K + 1 entries each, the sharp level last - hop, timepoints, scores (K + 1, n, 2)
    and labels_<k> for level k (labels_sharp for the sharp one); one line per level is printed and the same data is returned as
    a dict per file. Files are grouped like EvaluateCutoffSweep groups them - one framerate and sample type per call, up to 16
    files, a group cut short where its levels would take more than 8 GiB. hop=None is hop 1. accuracy= and resample= as in
    EvaluateNoiseSweep: confusion (K + 1, 2, 2) and accuracy_vtr (K + 1) per file that has its .FB / .PHN, framerate and
    source_framerate. The arguments are checked before any file is read."""
    from ... import smear
    if isinstance(files, (str, bytes, os.PathLike)):
        files = [files]
    spread, counts, names = SmearLevels(spreads, bands, F2Config().nchannels)
    matrices = {}                                 # per (framerate, channels)

    def call(ctx, handle, flat, dt, offsets, coefs, B, Cn, radius, STEP, hop, framerate, labels):
        if (framerate, Cn) not in matrices:
            freqs = filters.centre_freqs(framerate, Cn, F2Config().low_freq)
            matrices[framerate, Cn] = numpy.stack([smear.SmearMatrix(freqs, v) for v in spread] +
                                                  [smear.BandMatrix(Cn, v) for v in counts])
        scores = numpy.empty((len(labels), 2), numpy.float32)
        wo, stats = ctx.eval_smear_sweep(handle, flat, dt, offsets, coefs, B, Cn, bool(LPF), CUTOFF if LPF else 0.0, FFT_PRECISION,
                                         radius, STEP, hop, matrices[framerate, Cn], None, scores, labels, _lib.MEM_HOST)
        return wo, stats, None, scores

    def own(scores, rows, wo, n, radius, STEP, hop, framerate):
        return dict(spread_erb=numpy.concatenate([spread, numpy.full(len(counts), numpy.nan)]),
                    bands=numpy.concatenate([numpy.zeros(len(spread), numpy.int64), counts]),
                    timepoints=_lib.strided_timepoints(n, radius, STEP, hop), scores=numpy.stack([scores[wo[u]:wo[u + 1]] for u in rows]))

    axis = _SweepAxis(names=names, referee='sharp',
                      label="smear {:>8}", limit=LEVELS_LIMIT, call=call, own=own,
                      order=('spread_erb', 'bands', 'windows', 'rising', 'agree', 'agreement', 'hop', 'timepoints', 'scores'),
                      out=lambda file: os.path.splitext(file)[0] + '.smearsweep.npz', outdir=None, wav_target=None)
    return _run_sweep(axis, files, hop, model, ctx, accuracy, resample)
