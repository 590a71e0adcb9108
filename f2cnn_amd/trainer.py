"""The training state of ``cnn train --engine hip`` (include/f2cnn_hip.h: f2_trainer_*): master weights, RMSprop accumulators and
the training windows live on the device; a step is the recorded float32 forward in training mode, the backward chain with the
weight-gradient kernels, the optimiser and the refresh of the layouts the kernels read, all enqueued without a host round trip.

    t = Trainer(F2CNNModel.glorot(seed, rows, channels), lr=1e-4, decay=1e-6, drop=(0.25, 0.25, 0.5), seed=seed)
    t.set_data(x_train, y_train)                      # normalised float32 windows, 0 / 1 labels
    loss_sum, hits = t.steps(permutation, batch)      # one epoch: ceil(len / batch) steps, one wait
    model = t.model()                                 # the weights as an F2CNNModel
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
