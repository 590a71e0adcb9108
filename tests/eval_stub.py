"""A context that stands in for the device under `cnn eval`, `evalnoise` and `evalrand` (tests/test_eval_drivers.py,
tools/eval_drivers_old_new.py; not a test). Every output is a fixed function of the utterance - known by its length, so that a file
gets the same numbers alone and in a group - and of the row: labels come in blocks of BLOCK rows, the smoothed path equals the
labels, pictures and maps are reduced from those rows by plain numpy. Every call returns what the method of _lib.Context returns
and is logged as (method, B, lengths, dtype, hop, step, lpf, cutoff, width, K); for the stage calls on rows B counts the
utterances, lengths their rows, and what a call does not take is None."""
import numpy as np

from f2cnn_amd import _lib

BLOCK = 24


def _rows(N, nb):
    """(P(rising) float32, labels uint8) of the nb rows of an utterance of N samples"""
    j = np.arange(nb)
    lab = ((j // BLOCK + N) % 2).astype(np.uint8)
    p = np.where(lab == 1, 0.7, 0.2) + 0.01 * ((7 * j + N) % 10)
    return p.astype(np.float32), lab


def _emissions(p):
    return np.rint(65536.0 * np.log(p.astype(np.float64) / (1.0 - p.astype(np.float64)))).astype(np.int32)


def _columns(nb, N, origin, hop, width):
    """the time column of every row: its centre sample's share of [0, N)"""
    t = origin + np.arange(nb, dtype=np.int64) * hop
    return np.minimum(t * width // max(N, 1), width - 1)


def _column_means(values, col, width):
    """(rows per column (W), mean of values (nb, ...) per column (W, ...), NaN where a column has no row)"""
    values = np.asarray(values, np.float64)
    rows = np.bincount(col, minlength=width).astype(np.float64)
    out = np.full((width,) + values.shape[1:], np.nan)
    for x in np.flatnonzero(rows):
        out[x] = values[col == x].mean(axis=0)
    return rows, out


class StubContext:
    def __init__(self):
        self.calls = []

    def _log(self, method, B=None, lengths=None, dtype=None, hop=None, step=None, lpf=None, cutoff=None, width=None, K=None):
        self.calls.append((method, B, None if lengths is None else [int(n) for n in lengths], dtype, hop, step, lpf, cutoff, width, K))

    def cnn_create(self, tensors, rows, channels):
        return 1

    # ---- the evaluations ----------------------------------------------------------------------------------------------------
    def _evaluate(self, method, handle, wave, offsets, B, radius, step, hop, scores, labels, mem_space, every_sample=False):
        """fills scores (n, 2) / labels (n); returns (lengths, window_offsets)"""
        assert handle == 1 and mem_space == _lib.MEM_HOST and len(offsets) == B + 1 and wave.shape[0] == offsets[-1], method
        lengths = np.diff(offsets)
        nbs = [max(int(N) - (2 * radius + 1) * step, 0) if every_sample else _lib.strided_window_count(int(N), radius, step, hop)
               for N in lengths]
        wo = np.concatenate([[0], np.cumsum(nbs)]).astype(np.int64)
        assert scores.shape == (wo[-1], 2) and labels.shape == (wo[-1],), method
        for b, N in enumerate(lengths):
            p, lab = _rows(int(N), nbs[b])
            scores[wo[b]:wo[b + 1], 1], scores[wo[b]:wo[b + 1], 0] = p, np.float32(1) - p
            labels[wo[b]:wo[b + 1]] = lab
        return lengths, wo

    def eval_utterance(self, handle, wave, wave_dtype, N, coefs, Cn, lpf, cutoff, precision, radius, step, env, scores, labels, mem_space):
        self._log("eval_utterance", 1, [N], wave_dtype, None, step, lpf, cutoff)
        _, wo = self._evaluate("eval_utterance", handle, wave, np.array([0, N]), 1, radius, step, 1, scores, labels, mem_space, True)
        if env is not None:
            env[...] = 1.0
        return int(wo[-1])

    def eval_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, scores, labels, mem_space):
        self._log("eval_batch", B, np.diff(offsets), wave_dtype, None, step, lpf, cutoff)
        self._evaluate("eval_batch", handle, wave, offsets, B, radius, step, 1, scores, labels, mem_space, True)

    def eval_batch_strided(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, scores,
                           labels, mem_space):
        self._log("eval_batch_strided", B, np.diff(offsets), wave_dtype, hop, step, lpf, cutoff)
        return self._evaluate("eval_batch_strided", handle, wave, offsets, B, radius, step, hop, scores, labels, mem_space)[1]

    @staticmethod
    def _picture(levels, lengths):
        B, Cn, W = levels.shape
        for b, N in enumerate(lengths):
            levels[b] = (3 * np.arange(Cn)[:, None] + 5 * np.arange(W)[None, :] + int(N)) % 256
        return np.stack([np.zeros(B), np.asarray(lengths, np.float64)], axis=1)

    def eval_figure_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, spans, width,
                          pool, levels, track, scores, labels, mem_space, range_out=None):
        self._log("eval_figure_batch", B, np.diff(offsets), wave_dtype, hop, step, lpf, cutoff, width)
        assert spans is None and pool == 0 and levels.shape == (B, Cn, width) and track.shape == (B, width, 5)
        lengths, wo = self._evaluate("eval_figure_batch", handle, wave, offsets, B, radius, step, hop, scores, labels, mem_space)
        self._track(scores, labels, wo, lengths, radius * step, hop, width, track)
        return wo, self._picture(levels, lengths)

    def eval_occlusion_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, patches,
                             fill, spans, width, pool, levels, map_out, summary, scores, labels, mem_space, range_out=None):
        K = len(patches)
        self._log("eval_occlusion_batch", B, np.diff(offsets), wave_dtype, hop, step, lpf, cutoff, width, K)
        assert spans is None and pool == 0 and map_out.shape == (B, K, width, 4) and summary.shape == (B, K, 4)
        assert scores.shape[1:] == (K + 1, 2) and labels.shape[1:] == (K + 1,)
        base, lab = np.empty((len(scores), 2), np.float32), np.empty(len(scores), np.uint8)
        lengths, wo = self._evaluate("eval_occlusion_batch", handle, wave, offsets, B, radius, step, hop, base, lab, mem_space)
        for b, N in enumerate(lengths):
            rows = slice(wo[b], wo[b + 1])
            j = np.arange(wo[b + 1] - wo[b])
            p = base[rows, 1][:, None] + np.float32(0.05) * ((j[:, None] + np.arange(K + 1)[None, :] * (int(N) % 7 + 1)) % 5 - 2).astype(np.float32)
            p[:, 0] = base[rows, 1]
            scores[rows, :, 1], scores[rows, :, 0] = p, np.float32(1) - p
            labels[rows] = p > 0.5
            d = (p[:, 1:].astype(np.float64) - p[:, :1].astype(np.float64))
            flips = (labels[rows, 1:] != labels[rows, :1]).astype(np.float64)
            cells = np.stack([flips, d, np.abs(d)], axis=2)                          # (nb, K, 3)
            for w, out in ((width, map_out[b]), (1, summary[b].reshape(K, 1, 4))):
                count, mean = _column_means(cells, _columns(len(j), int(N), radius * step, hop, w), w)
                out[:, :, 0] = count[None, :]
                out[:, :, 1] = np.nan_to_num(mean[:, :, 0].T) * count[None, :]
                out[:, :, 2:] = mean[:, :, 1:].transpose(1, 0, 2)
        return wo, self._picture(levels, lengths)

    def eval_saliency_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, spans, width,
                            pool, levels, map_out, summary, scores, labels, mem_space, range_out=None):
        self._log("eval_saliency_batch", B, np.diff(offsets), wave_dtype, hop, step, lpf, cutoff, width)
        assert spans is None and pool == 0 and map_out.shape == (B, Cn, width, 3) and summary.shape == (B, Cn, 3)
        lengths, wo = self._evaluate("eval_saliency_batch", handle, wave, offsets, B, radius, step, hop, scores, labels, mem_space)
        for b, N in enumerate(lengths):
            j = np.arange(wo[b + 1] - wo[b])
            gx = ((3 * j[:, None] + 7 * np.arange(Cn)[None, :] + int(N)) % 11 - 5) / 100.0
            profile = np.stack([gx, np.abs(gx) + 0.01], axis=2)                      # (nb, Cn, 2)
            for w, out in ((width, map_out[b]), (1, summary[b].reshape(Cn, 1, 3))):
                count, mean = _column_means(profile, _columns(len(j), int(N), radius * step, hop, w), w)
                out[:, :, 0] = count[None, :]
                out[:, :, 1:] = mean.transpose(1, 0, 2)
        return wo, self._picture(levels, lengths)

    def eval_segments_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, logit_scale,
                            penalty, iv_offsets, iv_bounds, scores, labels, path, emissions, runs, tally, mem_space, want_value=True,
                            want_runs=True):
        self._log("eval_segments_batch", B, np.diff(offsets), wave_dtype, hop, step, lpf, cutoff, None, len(iv_bounds))
        _, wo = self._evaluate("eval_segments_batch", handle, wave, offsets, B, radius, step, hop, scores, labels, mem_space)
        value = self._path(scores, wo, path, emissions)
        ro = self._runs(path, emissions, wo, runs)
        self._tally(labels, path, emissions, wo, iv_offsets, iv_bounds, radius * step, hop, tally)
        return wo, value, ro

    # ---- the stage calls on rows --------------------------------------------------------------------------------------------
    @staticmethod
    def _track(scores, labels, wo, lengths, origin, hop, width, track):
        for u, N in enumerate(lengths):
            nb = int(wo[u + 1] - wo[u])
            col = _columns(nb, int(N), origin, hop, width)
            p = scores[wo[u]:wo[u + 1], 1].astype(np.float64)
            count, mean = _column_means(np.stack([labels[wo[u]:wo[u + 1]], p], axis=1), col, width)
            track[u, :, 0], track[u, :, 1], track[u, :, 2] = count, np.nan_to_num(mean[:, 0]) * count, mean[:, 1]
            track[u, :, 3:] = np.nan
            for x in np.flatnonzero(count):
                track[u, x, 3], track[u, x, 4] = p[col == x].min(), p[col == x].max()
        return track

    def score_track(self, scores, labels, window_offsets, spans, origin, hop, width, track, mem_space):
        self._log("score_track", len(window_offsets) - 1, np.diff(window_offsets), None, hop, None, None, None, width)
        spans = np.asarray(spans).reshape(-1, 2)
        assert mem_space == _lib.MEM_HOST and (spans[:, 0] == 0).all() and track.shape == (len(spans), width, 5)
        return self._track(scores, labels, window_offsets, spans[:, 1], origin, hop, width, track)

    @staticmethod
    def _path(scores, wo, path, emissions):
        q = _emissions(scores[:, 1])
        path[...] = q > 0
        if emissions is not None:
            emissions[...] = q
        return np.array([np.abs(q[wo[u]:wo[u + 1]].astype(np.int64)).sum() for u in range(len(wo) - 1)], np.int64)

    def decision_path(self, scores, window_offsets, logit_scale, penalty, path, mem_space, emissions=None, value=None):
        self._log("decision_path", len(window_offsets) - 1, np.diff(window_offsets))
        assert mem_space == _lib.MEM_HOST
        return self._path(scores, window_offsets, path, emissions)

    @staticmethod
    def _runs(labels, emissions, wo, runs):
        ro, at = [0], 0
        for u in range(len(wo) - 1):
            lab, q = labels[wo[u]:wo[u + 1]], emissions[wo[u]:wo[u + 1]].astype(np.int64)
            starts = np.flatnonzero(np.concatenate([[True], lab[1:] != lab[:-1]])) if len(lab) else np.zeros(0, np.int64)
            ends = np.concatenate([starts[1:], [len(lab)]]) if len(lab) else starts
            for a, e in zip(starts, ends):
                runs.reshape(-1, 4)[at] = a, e - a, lab[a], q[a:e].sum()
                at += 1
            ro.append(at)
        return np.array(ro, np.int64)

    def decision_runs(self, labels, emissions, window_offsets, runs, capacity, mem_space, run_offsets=None):
        self._log("decision_runs", len(window_offsets) - 1, np.diff(window_offsets))
        assert mem_space == _lib.MEM_HOST and capacity == len(labels)
        return self._runs(labels, emissions, window_offsets, runs)

    @staticmethod
    def _tally(labels, path, emissions, wo, ivo, ivb, origin, hop, tally):
        U, R = len(wo) - 1, len(ivo) - 1
        assert U == R, "the drivers give one interval set per utterance"
        ivb = np.asarray(ivb).reshape(-1, 2)
        for u in range(U):
            t = origin + np.arange(wo[u + 1] - wo[u], dtype=np.int64) * hop
            rows = slice(wo[u], wo[u + 1])
            for i in range(ivo[u], ivo[u + 1]):
                m = (t >= ivb[i, 0]) & (t < ivb[i, 1])
                tally.reshape(-1, 4)[i] = m.sum(), labels[rows][m].sum(), path[rows][m].sum(), emissions[rows][m].astype(np.int64).sum()
        return tally

    def interval_tally(self, labels, path, emissions, window_offsets, iv_offsets, iv_bounds, origin, hop, tally, mem_space):
        self._log("interval_tally", len(window_offsets) - 1, np.diff(window_offsets), None, hop, None, None, None, None, len(iv_bounds))
        assert mem_space == _lib.MEM_HOST
        return self._tally(labels, path, emissions, window_offsets, iv_offsets, iv_bounds, origin, hop, tally)

    def label_accuracy(self, labels, window_offsets, ref_offsets, ref_timepoints, ref_signs, origin, hop, step, mem_space, counts=None):
        wo = np.asarray(window_offsets, np.int64)
        U, R = len(wo) - 1, len(ref_offsets) - 1
        self._log("label_accuracy", U, np.diff(wo), None, hop, step, None, None, None, R)
        assert mem_space == _lib.MEM_HOST and len(labels) == wo[-1]
        counts = np.zeros((U, 2, 2), np.int64)
        for u in range(U):
            r = u % R
            for t, s in zip(ref_timepoints[ref_offsets[r]:ref_offsets[r + 1]], ref_signs[ref_offsets[r]:ref_offsets[r + 1]]):
                j = (int(t) - origin + hop // 2) // hop
                if 0 <= j < wo[u + 1] - wo[u]:
                    counts[u, int(s), int(labels[wo[u] + j])] += 1
        return counts


# ---- the corpus and the runs of the three commands under the stub -----------------------------------------------------------
WIDTH = 64
OPTION_SETS = {                                   # name -> keywords of the three functions
    "none": {},
    "figure": dict(figure=True),
    "occlusion": dict(occlusion=True),
    "occlusion+figure": dict(occlusion=True, figure=True),
    "saliency": dict(saliency=True),
    "saliency+figure": dict(saliency=True, figure=True),
    "segments": dict(segments=True),
    "segments+figure": dict(segments=True, figure=True),
    "segments+occlusion": dict(segments=True, occlusion=True),
    "segments+saliency+figure": dict(segments=True, saliency=True, figure=True),
}
COMMANDS = ("eval", "evalnoise", "evalrand")
# (option set, accuracy, hop): every set at hop 160 without and with accuracy='centre'; none and segments at hop None as well
MATRIX = [(name, accuracy, 160) for name in OPTION_SETS for accuracy in (None, "centre")] + \
         [(name, accuracy, None) for name in ("none", "segments") for accuracy in (None, "centre")]


def build_corpus(root):
    """configF2CNN.conf, model.npz and resources/f2cnn/TEST/ with a labelled file of 19 200 samples (.FB, .PHN of four phonemes), a
    bare file of 4000 samples and an 8 kHz RIFF file of 2000 samples, which makes every group of `evalrand` a mixed one. Returns
    the three paths, relative to root, in that order."""
    import os
    from scipy.io import wavfile
    import label_referee
    from f2cnn_amd import config, wavio
    from f2cnn_amd.model import F2CNNModel
    root = str(root)
    config.write_default(os.path.join(root, "configF2CNN.conf"))
    folder = os.path.join(root, "resources", "f2cnn", "TEST")
    os.makedirs(folder)
    rng = np.random.default_rng(45)
    wave = lambda n: (3000 * rng.standard_normal(n)).astype(np.int16)
    label_referee.write_labelled_file(folder, wave)
    with open(os.path.join(folder, "DR1.FSYN0.SA1.PHN"), "w") as f:
        f.write("0 3000 h#\n3000 9000 aa\n9000 14000 t\n14000 19200 aa\n")
    wavio.write_sphere(os.path.join(folder, "BARE.WAV"), 16000, wave(4000))
    wavfile.write(os.path.join(folder, "RIFF8K.WAV"), 8000, wave(2000))
    F2CNNModel.glorot(7).save(os.path.join(root, "model.npz"))
    return [os.path.join("resources", "f2cnn", "TEST", name + ".WAV") for name in ("DR1.FSYN0.SA1", "BARE", "RIFF8K")]


def _cli_arguments(file, options, accuracy, hop):
    argv = ["cnn", "eval", "-f", file, "-m", "model.npz"]
    argv += [] if hop is None else ["--hop", str(hop)]
    argv += [] if accuracy is None else ["--accuracy", accuracy]
    argv += ["--" + name for name in ("figure", "occlusion", "saliency", "segments") if name in options]
    return argv + (["--figure-width", str(WIDTH)] if set(options) - {"segments"} else [])


def run_function(root, call):
    """call() in `root`, cleared of earlier outputs, under a fresh stub: a dict - returned (what it returned), stdout, log, error
    ((type name, message) or None), npz {path: {key: array}, keys in stored order} and png {path: bytes} of what it wrote"""
    import contextlib, glob, io, os, shutil
    import pytest
    here = os.getcwd()
    os.chdir(str(root))
    try:
        for stale in glob.glob(os.path.join("resources", "f2cnn", "TEST", "*.F2CNN.npz")) + ["graphs", "OutputWavFiles"]:
            shutil.rmtree(stale) if os.path.isdir(stale) else os.path.exists(stale) and os.remove(stale)
        stub, text, error, returned = StubContext(), io.StringIO(), None, None
        state = np.random.get_state()
        np.random.seed(45)                         # (evalrand permutes its files)
        with pytest.MonkeyPatch.context() as patch, contextlib.redirect_stdout(text):
            patch.setattr(_lib, "default_context", lambda: stub)
            try:
                returned = call()
            except Exception as e:                 # (recorded: the same on both trees)
                error = (type(e).__name__, str(e))
            finally:
                np.random.set_state(state)
        written = sorted(glob.glob(os.path.join("**", "*.F2CNN.npz"), recursive=True))
        pictures = sorted(glob.glob(os.path.join("graphs", "**", "*.png"), recursive=True))
        return dict(returned=returned, stdout=text.getvalue(), log=stub.calls, error=error,
                    npz={path: dict(np.load(path)) for path in written}, png={path: open(path, "rb").read() for path in pictures})
    finally:
        os.chdir(here)


def run_command(root, command, options, accuracy, hop, files, model="model.npz"):
    """One command over the corpus, each call of it through run_function - `eval` through cli.main and `evalnoise` through its
    function once per file, `evalrand` once: the list of run_function's dicts, each with `files`, those of the call in the order they
    were evaluated"""
    from f2cnn_amd import cli
    from f2cnn_amd.scripts.CNN import Evaluating
    keywords = dict(options, hop=hop, accuracy=accuracy, model=model, figure_width=WIDTH)
    if command == "evalrand":
        out = run_function(root, lambda: Evaluating.EvaluateRandom(**keywords))
        return [dict(out, files=list(out["returned"] or files))]
    if command == "eval":
        return [dict(run_function(root, lambda: cli.main(_cli_arguments(f, options, accuracy, hop))), files=[f]) for f in files]
    return [dict(run_function(root, lambda: Evaluating.EvaluateWithNoise(f, SNRdB=10, rng=np.random.default_rng(5), **keywords)), files=[f])
            for f in files]
