"""The training state of ``cnn train --engine hip`` (include/f2cnn_hip.h: f2_trainer_*): master weights, RMSprop accumulators and
the training windows live on the device; a step is the recorded float32 forward in training mode, the backward chain with the
weight-gradient kernels, the optimiser and the refresh of the layouts the kernels read, all enqueued without a host round trip.

    t = Trainer(F2CNNModel.glorot(seed, rows, channels), lr=1e-4, decay=1e-6, drop=(0.25, 0.25, 0.5), seed=seed)
    t.set_data(x_train, y_train)                      # normalised float32 windows, 0 / 1 labels
    loss_sum, hits = t.steps(permutation, batch)      # one epoch: ceil(len / batch) steps, one wait
    model = t.model()                                 # the weights as an F2CNNModel

A trainer can own the waves instead of the windows and rebuild the windows under new noise before every epoch:

    t.set_waves(waves, centers, signs, coefs, radius=5, step=160)   # one array of samples and of centres per utterance
    t.render(snrs=(20, 10), level_of=levels, seed=s)                # utterance b at snrs[levels[b]], len(snrs) = clean
    t.render_wet(rirs=[h0, h1], room_of=rooms, snrs=(20, 10), level_of=levels, seed=s)   # ... in room rirs[rooms[b]] first
    t.render(snrs=(20, 10), level_of=levels, seed=s, firs=[pink, speech])   # ... under noise of the colour firs[levels[b]]
    t.render(snrs=(20, 10), level_of=levels, seed=s, cutoffs=(5, 50), cutoff_of=cut)   # ... envelopes low-passed at cutoffs[cut[b]] Hz
    x, y = t.windows()                                              # what the network is about to see
"""
import numpy as np

from . import _lib
from .model import NAMES, F2CNNModel, tensor_shapes


class Trainer:
    def __init__(self, model, lr=1e-4, rho=0.9, eps=1e-7, decay=1e-6, drop=(0.25, 0.25, 0.5), seed=0, ctx=None):
        self.ctx = ctx or _lib.default_context()
        self.rows, self.channels = model.rows, model.channels
        self.names = [n + s for n in NAMES for s in ("_w", "_b")]
        shapes = tensor_shapes(self.rows, self.channels)
        self.shapes = [shapes[k] for k in self.names]
        self.handle = self.ctx.trainer_create(model.ordered(), self.rows, self.channels, lr, rho, eps, decay, drop, seed)

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.ctx.trainer_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, x, y):
        x = np.asarray(x)
        if x.ndim == 4 and x.shape[-1] == 1:
            x = x[..., 0]
        if x.ndim != 3 or x.shape[1:] != (self.rows, self.channels):
            raise ValueError(f"expected windows of shape (n,{self.rows},{self.channels}[,1]), got {x.shape}")
        y = np.asarray(y).reshape(-1)
        if len(y) != len(x) or (len(y) and (y.min() < 0 or y.max() > 1)):
            raise ValueError("y holds one sign, 0 (falling) or 1 (rising), per window")
        self.ctx.trainer_set_data(self.handle, x, y)

    def set_waves(self, waves, centers, signs, coefs, radius, step, lpf=False, cutoff=50.0, precision=None, group=64):
        """The corpus the windows are rendered from: `waves` one int16 or float64 array per utterance, `centers` / `signs` one array
        per utterance of window centres (samples from the utterance's start) and of 0 / 1 labels. Replaces set_data's windows."""
        waves = [np.ascontiguousarray(w).reshape(-1) for w in waves]
        if len(centers) != len(waves) or len(signs) != len(waves):
            raise ValueError("centers and signs hold one array per utterance")
        f64 = any(w.dtype != np.int16 for w in waves)
        dtype = np.float64 if f64 else np.int16
        wave = np.concatenate([w.astype(dtype, copy=False) for w in waves]) if waves else np.zeros(0, dtype)
        offsets = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
        cen = [np.asarray(c, dtype=np.int64).reshape(-1) for c in centers]
        sg = [np.asarray(g).reshape(-1) for g in signs]
        if any(len(c) != len(g) for c, g in zip(cen, sg)):
            raise ValueError("every centre has one sign")
        center_offsets = np.concatenate([[0], np.cumsum([len(c) for c in cen])]).astype(np.int64)
        flat = np.concatenate(cen) if cen else np.zeros(0, np.int64)
        y = np.concatenate(sg) if sg else np.zeros(0, np.uint8)
        if len(y) and (y.min() < 0 or y.max() > 1):
            raise ValueError("signs are 0 (falling) or 1 (rising)")
        coefs = np.ascontiguousarray(coefs, dtype=np.float64)
        self.ctx.trainer_set_waves(self.handle, wave, _lib.WAVE_F64 if f64 else _lib.WAVE_I16, offsets, coefs, len(waves), coefs.shape[0],
                                   lpf, cutoff, _lib.FFT_F32 if precision is None else precision, center_offsets, flat,
                                   y.astype(np.uint8), int(radius), int(step), group)

    def _render(self, wet, rirs, room_of, snrs, level_of, seed, firs, mixes, mix_of, maskers=None, masker_of=None, masker_snrs=(),
                masker_level_of=None, cutoffs=None, cutoff_of=None):
        """the entry of render (wet False: no rooms) / render_wet: the lowest that has every stage asked for"""
        if cutoffs is not None:
            self.ctx.trainer_render_filtered(self.handle, rirs, room_of, snrs, firs, level_of, seed, mixes, mix_of, self.channels, maskers,
                                             masker_of, masker_snrs, masker_level_of, cutoffs, cutoff_of)
        elif maskers is not None:
            self.ctx.trainer_render_masked(self.handle, rirs, room_of, snrs, firs, level_of, seed, mixes, mix_of, self.channels, maskers,
                                           masker_of, masker_snrs, masker_level_of)
        elif mixes is not None:
            self.ctx.trainer_render_smeared(self.handle, rirs, room_of, snrs, firs, level_of, seed, mixes, mix_of, self.channels)
        elif firs is not None:
            self.ctx.trainer_render_coloured(self.handle, rirs, room_of, snrs, firs, level_of, seed)
        elif wet:
            self.ctx.trainer_render_wet(self.handle, rirs, room_of, snrs, level_of, seed)
        else:
            self.ctx.trainer_render(self.handle, snrs, level_of, seed)

    def render(self, snrs=(), level_of=None, seed=0, firs=None, mixes=None, mix_of=None, maskers=None, masker_of=None, masker_snrs=(),
               masker_level_of=None, cutoffs=None, cutoff_of=None):
        """Rebuild the training windows from the stored waves: utterance b at snrs[level_of[b]] dB, clean where level_of[b] ==
        len(snrs) or level_of is None; the noise of an utterance depends on (seed, its level, its number) alone. firs (one 1-D
        float64 filter per level): the noise of level l is filtered with firs[l] (f2_trainer_render_coloured); None: white.
        mixes ((K, C, C) float64) and mix_of: the windows of utterance b are mixed across their channels by mixes[mix_of[b]]
        before they are normalised, sharp where mix_of[b] == K (f2_trainer_render_smeared); None: the render without them.
        maskers (1-D float64 recordings), masker_of (the recording of each masker level), masker_snrs (its SNR) and masker_level_of:
        utterance b is mixed with a segment of maskers[masker_of[l]] at masker_snrs[l] dB, l = masker_level_of[b], before the noise;
        no masker where l == len(masker_snrs) (f2_trainer_render_masked); None: the render without them.
        cutoffs (Hz) and cutoff_of: the unfiltered envelopes of utterance b are low-passed at cutoffs[cutoff_of[b]] before the
        windows are gathered, left unfiltered where cutoff_of[b] == len(cutoffs) (f2_trainer_render_filtered); the waves must have
        been set with lpf=False. None: the render without them."""
        self._render(False, (), None, snrs, level_of, seed, firs, mixes, mix_of, maskers, masker_of, masker_snrs, masker_level_of, cutoffs,
                     cutoff_of)

    def render_wet(self, rirs=(), room_of=None, snrs=(), level_of=None, seed=0, firs=None, mixes=None, mix_of=None, maskers=None,
                   masker_of=None, masker_snrs=(), masker_level_of=None, cutoffs=None, cutoff_of=None):
        """render() with a room per utterance: utterance b is convolved with rirs[room_of[b]] (float64 arrays), dry where
        room_of[b] == len(rirs) or room_of is None, and then noised at snrs[level_of[b]] dB of the reverberant signal. Without
        rooms it is render(), bit for bit. firs, mixes, mix_of, the maskers (which stay dry), cutoffs and cutoff_of: as in render()."""
        self._render(True, rirs, room_of, snrs, level_of, seed, firs, mixes, mix_of, maskers, masker_of, masker_snrs, masker_level_of,
                     cutoffs, cutoff_of)

    def windows(self, first=0, count=None):
        """(x, y): rows first .. first + count - 1 of the training set as it stands on the device (count None: to the end)"""
        n = int(self.ctx.trainer_info(self.handle, "windows"))
        count = n - first if count is None else count
        return self.ctx.trainer_get_windows(self.handle, first, count, (self.rows, self.channels))

    def steps(self, order, batch):
        """(loss sum, windows decided as labelled) over the steps, each with the weights it started from"""
        return self.ctx.trainer_steps(self.handle, order, batch)

    def _get(self, what):
        return dict(zip(self.names, self.ctx.trainer_get(self.handle, what, self.shapes)))

    def weights(self):
        return self._get("weights")

    def accumulators(self):
        return self._get("accumulators")

    def gradient(self):
        """the last step's gradient of the summed loss (before the division by the step's window count)"""
        return self._get("gradient")

    def model(self):
        return F2CNNModel(self.weights(), self.rows, self.channels)

    @property
    def iterations(self):
        return int(self.ctx.trainer_info(self.handle, "iterations"))
