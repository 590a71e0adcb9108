"""Counterpart of the reference's ``scripts/CNN/Training.py``.

``normalizeInput`` (:13-28) is on the hot path and runs through HIP kernel K3. ``SeparateTestTrain`` (:31-44) and
``TrainAndPlotLoss`` (:47-156) are SURVEY section 8f row n4: the same network (:93-114; weights in
``f2cnn_amd.model``), RMSprop(lr 1e-4, decay 1e-6), categorical cross-entropy, early stopping on the validation
accuracy (min_delta 0.01, patience 5), trained with PyTorch-ROCm autograd as the scope table asks, or (``engine='hip'``,
``cnn train --engine hip``) with the library's own training step: weight gradients, dropout and RMSprop on the device. Training only
produces weights; every forward pass used for evaluation is HIP kernel K4 (the trained weights are written in the
``.npz`` container K4 loads, under the reference's file name ``last_trained_model``).

``TrainFromWav`` (`cnn train --engine hip --from-wav`, not in the reference) trains on windows the device renders from the WAV files,
again before every epoch under fresh noise (``--augment-snrs``), of a colour drawn per file (``--augment-colours``), and in a
freshly drawn room per file (``--augment-t60``, ``--augment-rirs``) and at a spectral resolution drawn per file
(``--augment-spreads``, ``--augment-bands``) and under a recorded masker drawn per file (``--augment-maskers``) and with the
envelopes low-passed at a cutoff drawn per file (``--augment-cutoffs``) when asked.

``TestModel`` (`cnn test`, not in the reference) is ``model.evaluate(x_test, y_test)`` (:136) for a saved model, broken down
by a column of the label CSV: one ``f2_cnn_score_windows`` call on the stored windows.
"""
import csv
import json
import os

import numpy

from ... import _lib


def normalizeInput(matrix, ctx=None):
    """Per-window log min-max normalisation: (ln x - ln min)/(ln max - ln min); a constant window gives
    zeros; any value <= 0 raises ValueError("values must all be positive"). Same dtype and shape out.
    Runs on the GPU through the window kernel (one window, step 1)."""
    ctx = ctx or _lib.default_context()
    m = numpy.asarray(matrix)
    shape, dtype = m.shape, m.dtype
    if m.ndim < 2:
        raise ValueError("matrix must be at least two dimensional")
    rows = shape[0]
    flat = numpy.ascontiguousarray(m.reshape(rows, -1), dtype=numpy.float64)
    if rows % 2 == 0:   # the kernel takes 2*radius+1 rows; pad an even window with a copy of its last row
        flat = numpy.vstack([flat, flat[-1:]])
    R, Cn = flat.shape
    env = numpy.ascontiguousarray(flat.T)           # (C, N=R): env[c, k]
    out = numpy.empty((1, R, Cn), numpy.float32)
    try:
        ctx.gather_windows(env, Cn, R, numpy.array([R // 2], numpy.int64), 1, R // 2, 1, True, out, _lib.MEM_HOST)
    except _lib.F2Error as e:
        if e.code == _lib.F2_ERR_NONPOSITIVE:
            print(shape)
            raise ValueError("values must all be positive")
        raise
    res = out[0, :rows].reshape(shape)
    return res.astype(dtype) if numpy.issubdtype(dtype, numpy.floating) else res.astype(numpy.float64)


def normalizeInputBatch(windows, ctx=None):
    """normalizeInput applied to every (rows, C) window of an (n, rows, C) array in one K3 launch; float32 out.
    (The reference loops over the windows, Training.py:72-75. It casts to float32 *before* taking logarithms there;
    K3 takes them in float64 and rounds once, the convention of the evaluation path, Evaluating.py:66-68.)"""
    ctx = ctx or _lib.default_context()
    w = numpy.asarray(windows)
    if w.ndim == 4 and w.shape[-1] == 1:
        w = w[..., 0]
    if w.ndim != 3 or w.shape[1] % 2 == 0:
        raise ValueError("expected (n, 2*radius+1, channels) windows")
    n, R, Cn = w.shape
    out = numpy.empty((n, R, Cn), numpy.float32)
    if n == 0:
        return out
    env = numpy.ascontiguousarray(w.reshape(n * R, Cn).T, dtype=numpy.float64)     # (C, n*R): the windows end to end
    centers = numpy.arange(n, dtype=numpy.int64) * R + R // 2
    try:
        ctx.gather_windows(env, Cn, n * R, centers, n, R // 2, 1, True, out, _lib.MEM_HOST)
    except _lib.F2Error as e:
        if e.code == _lib.F2_ERR_NONPOSITIVE:
            raise ValueError("values must all be positive")
        raise
    return out


def SeparateTestTrain(pathToInput, pathToLabel):
    """(x_test, y_test, x_train, y_train): row i of the label CSV goes with input_data[i]; first column 'TEST'
    selects the test set, the last column is the 0/1 sign (Training.py:31-44)."""
    x = [[], []]
    y = [[], []]
    input_data = numpy.load(pathToInput)
    with open(pathToLabel, 'r') as labels:
        for i, row in enumerate(csv.reader(labels)):
            test, sign = row[0], row[8]
            k = 0 if test == 'TEST' else 1
            x[k].append(input_data[i])
            y[k].append(int(sign))
    return numpy.array(x[0]), numpy.array(y[0]), numpy.array(x[1]), numpy.array(y[1])


def build_network(rows=11, channels=128):
    """The Sequential model of Training.py:93-114 as a torch module (NCHW); layer names match
    F2CNNModel.from_torch_state_dict. Keras defaults: glorot_uniform kernels, zero biases."""
    import torch
    from torch import nn
    from ...model import flatten_size

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(1, 32, 3, padding=1)      # padding='same'
            self.conv2 = nn.Conv2d(32, 32, 3)
            self.conv3 = nn.Conv2d(32, 64, 3, padding=1)
            self.conv4 = nn.Conv2d(64, 64, 3)
            self.dense1 = nn.Linear(flatten_size(rows, channels)[2], 516)
            self.dense2 = nn.Linear(516, 2)
            self.drop1, self.drop2, self.drop3 = nn.Dropout(0.25), nn.Dropout(0.25), nn.Dropout(0.5)
            for m in (self.conv1, self.conv2, self.conv3, self.conv4, self.dense1, self.dense2):
                nn.init.xavier_uniform_(m.weight)
                nn.init.zeros_(m.bias)

        def forward(self, x):                                  # logits; softmax lives in the loss / K4
            F = torch.nn.functional
            x = F.relu(self.conv1(x))
            x = self.drop1(F.max_pool2d(F.relu(self.conv2(x)), 2))
            x = F.relu(self.conv3(x))
            x = self.drop2(F.max_pool2d(F.relu(self.conv4(x)), 2))
            x = self.drop3(F.relu(self.dense1(torch.flatten(x, 1))))
            return self.dense2(x)

    return Net()


ENGINES = ("torch", "hip")
DROPOUT = (0.25, 0.25, 0.5)     # the three Dropout layers of Training.py:93-114


def _torch_engine(x_train, y_train, x_test, y_test, batch_size, device, seed, lr, decay):
    """PyTorch-ROCm autograd: (run_epoch() -> (loss sum, hits), validate() -> (val_loss, val_acc), export() -> F2CNNModel)"""
    import torch
    from ...model import F2CNNModel
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("cnn train needs a GPU (PyTorch-ROCm device); pass device='cpu' explicitly to override")
        device = "cuda"
    if seed is not None:
        torch.manual_seed(seed)
    rows, channels = x_train.shape[1], x_train.shape[2]
    net = build_network(rows, channels).to(device)
    xt = torch.from_numpy(x_train).unsqueeze(1).to(device)
    yt = torch.from_numpy(numpy.asarray(y_train, numpy.int64)).to(device)
    xv = torch.from_numpy(x_test).unsqueeze(1).to(device)
    yv = torch.from_numpy(numpy.asarray(y_test, numpy.int64)).to(device)
    opt = torch.optim.RMSprop(net.parameters(), lr=lr, alpha=0.9, eps=1e-7)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0 / (1.0 + decay * it))
    loss_fn = torch.nn.CrossEntropyLoss(reduction="sum")

    def evaluate(x, y):
        net.eval()
        tot, hit = 0.0, 0
        with torch.no_grad():
            for i in range(0, len(x), 1024):
                lg = net(x[i:i + 1024])
                tot += float(loss_fn(lg, y[i:i + 1024]))
                hit += int((lg.argmax(1) == y[i:i + 1024]).sum())
        n = max(len(x), 1)
        return tot / n, hit / n

    def run_epoch():
        net.train()
        perm = torch.randperm(len(xt), device=device)          # fit(shuffle=True)
        tot, hit = 0.0, 0
        for i in range(0, len(xt), batch_size):
            idx = perm[i:i + batch_size]
            lg = net(xt[idx])
            loss = loss_fn(lg, yt[idx])
            opt.zero_grad(set_to_none=True)
            (loss / len(idx)).backward()
            opt.step()
            sched.step()
            tot += float(loss.detach())
            hit += int((lg.argmax(1) == yt[idx]).sum())
        return tot, hit

    def validate():
        return evaluate(xv, yv) if len(xv) else (float("nan"), float("nan"))

    return run_epoch, validate, lambda: F2CNNModel.from_torch_state_dict(net.state_dict(), rows, channels)


def _hip_trainer(rows, channels, seed, lr, decay, ctx):
    """(Trainer, rng of the epochs' order): initial weights F2CNNModel.glorot(seed, zero_bias=True) (Keras' defaults), the masks'
    seed the run's; the same seed gives the same weights bit for bit"""
    from ...trainer import Trainer
    from ...model import F2CNNModel
    rng = numpy.random.default_rng(seed)
    mask_seed = int(seed) if seed is not None else int(rng.integers(0, 2 ** 63))
    trainer = Trainer(F2CNNModel.glorot(seed, rows, channels, zero_bias=True), lr=lr, rho=0.9, eps=1e-7, decay=decay, drop=DROPOUT,
                      seed=mask_seed, ctx=ctx)
    return trainer, rng


def _hip_validate(trainer, ctx, x_test, y_val, **groups):
    """F2CNNModel.evaluate (f2_cnn_score_windows) of the trainer's exported weights on the validation windows"""
    model = trainer.model()
    try:
        return model.evaluate(x_test, y_val, ctx=ctx, **groups)
    finally:
        model.release(ctx)


def _hip_engine(x_train, y_train, x_test, y_test, batch_size, seed, lr, decay, ctx=None):
    """The library's own training step (f2_trainer_*): weights, RMSprop accumulators and the training set stay on the device, an
    epoch is one f2_trainer_steps call over a NumPy permutation. Initial weights F2CNNModel.glorot(seed, zero_bias=True) (Keras'
    defaults); the same seed gives the same weights bit for bit. Validation goes through F2CNNModel.evaluate
    (f2_cnn_score_windows) on the exported weights."""
    ctx = ctx or _lib.default_context()       # (no library or no device: raises here)
    trainer, rng = _hip_trainer(x_train.shape[1], x_train.shape[2], seed, lr, decay, ctx)
    trainer.set_data(x_train, numpy.asarray(y_train))
    y_val = numpy.asarray(y_test)

    def validate():
        if not len(x_test):
            return float("nan"), float("nan")
        return _hip_validate(trainer, ctx, x_test, y_val)

    return lambda: trainer.steps(rng.permutation(len(x_train)), batch_size), validate, trainer.model


def train_network(x_train, y_train, x_test, y_test, batch_size=32, epochs=20, device=None, seed=None, verbose=1,
                  lr=1e-4, decay=1e-6, min_delta=0.01, patience=5, engine="torch"):
    """model.compile + model.fit of Training.py:117-135 on already normalised float32 windows (n, rows, C).
    Returns (F2CNNModel, history) with history = {'loss','acc','val_loss','val_acc'} per epoch.
    RMSprop as Keras 2.2 runs it: rho 0.9, epsilon 1e-7, lr_t = lr / (1 + decay * iterations).
    engine: 'torch' (PyTorch-ROCm autograd) or 'hip' (the library's own kernels, on the default context's device; `device` is
    not used). Both share the epoch loop and the early-stopping rule below."""
    if engine not in ENGINES:
        raise ValueError("engine must be one of {}, not {!r}".format(ENGINES, engine))
    x_train = numpy.asarray(x_train, numpy.float32)
    x_test = numpy.asarray(x_test, numpy.float32)
    if engine == "torch":
        run_epoch, validate, export = _torch_engine(x_train, y_train, x_test, y_test, batch_size, device, seed, lr, decay)
    else:
        run_epoch, validate, export = _hip_engine(x_train, y_train, x_test, y_test, batch_size, seed, lr, decay)
    return fit_epochs(run_epoch, validate, export, len(x_train), epochs, verbose, min_delta, patience)


def fit_epochs(run_epoch, validate, export, n_train, epochs, verbose=1, min_delta=0.01, patience=5):
    """The epoch loop and the early-stopping rule every engine shares: run_epoch() -> (loss sum, hits) over the n_train windows,
    validate() -> (val_loss, val_acc), export() -> F2CNNModel. Returns (export(), history)."""
    history = {"loss": [], "acc": [], "val_loss": [], "val_acc": []}
    best, wait = -numpy.inf, 0
    for epoch in range(epochs):
        tot, hit = run_epoch()
        vl, va = validate()
        for k, val in zip(("loss", "acc", "val_loss", "val_acc"), (tot / n_train, hit / n_train, vl, va)):
            history[k].append(val)
        if verbose:
            print("Epoch {}/{} - loss: {:.4f} - acc: {:.4f} - val_loss: {:.4f} - val_acc: {:.4f}".format(
                epoch + 1, epochs, history["loss"][-1], history["acc"][-1], vl, va))
        # keras.callbacks.EarlyStopping(monitor='val_acc', min_delta=0.01, patience=5, mode='auto')
        if va - min_delta > best:
            best, wait = va, 0
        else:
            wait += 1
            if wait >= patience:
                if verbose:
                    print("Epoch {:05d}: early stopping".format(epoch + 1))
                break
    return export(), history


class LabelledWaves:
    """The label CSV read once: per file, in sorted key order (the row order of `prepare input`), `wavs` its WAV path
    (wav_for_label_key), `centers` its timepoints in CSV order (int64), `signs` their 0 / 1 labels (uint8) and `is_test` whether its
    rows say TEST. A label key without its WAV raises FileNotFoundError here; read(reach) loads the audio and raises ValueError
    for a timepoint whose window leaves its file - both with GenerateInputDataFromWav's messages, before any device work."""

    def __init__(self, labelFile):
        from ..processing.InputGenerator import wav_for_label_key
        from ..processing.LabelDataGenerator import CSV_COLUMNS
        sign_col = CSV_COLUMNS.index('sign')
        per_file = {}
        with open(labelFile, 'r') as labels:
            for i, row in enumerate(csv.reader(labels)):
                if not row:
                    continue
                testOrTrain, region, speaker, sentence, _phoneme, timepoint = row[:6]
                sign = int(row[sign_col])
                if sign not in (0, 1):
                    raise ValueError("row {}: sign {!r} is neither 0 nor 1".format(i, row[sign_col]))
                key = os.path.join(testOrTrain, '.'.join((region, speaker, sentence, 'ENV1.npy')))
                entry = per_file.setdefault(key, ([], [], testOrTrain == 'TEST'))
                entry[0].append(int(timepoint))
                entry[1].append(sign)
        self.keys = sorted(per_file)
        self.wavs = [wav_for_label_key(key) for key in self.keys]
        self.centers = [numpy.array(per_file[key][0], numpy.int64) for key in self.keys]
        self.signs = [numpy.array(per_file[key][1], numpy.uint8) for key in self.keys]
        self.is_test = [per_file[key][2] for key in self.keys]
        for key, wav in zip(self.keys, self.wavs):
            if not os.path.isfile(wav):
                raise FileNotFoundError("{} (label key {}) does not exist".format(wav, key))

    def __len__(self):
        return len(self.keys)

    def read(self, reach):
        """The samples of every file (int16, or float64 where the file is not 16-bit), each window checked against its file"""
        from ...gammatone import filters
        from ..processing.GammatoneFiltering import GetArrayFromWAV
        waves = []
        for wav, centers in zip(self.wavs, self.centers):
            samples = filters._wave_args(GetArrayFromWAV(wav)[1])[0]
            n = samples.shape[0]
            for tp in centers:
                if tp - reach < 0 or tp + reach >= n:
                    raise ValueError("{}: the window at timepoint {} (+-{} samples) reaches outside its {} samples".format(
                        wav, int(tp), reach, n))
            waves.append(samples)
        return waves

    def split(self, test):
        """indices of the TEST (test=True) or the other files"""
        return [k for k, t in enumerate(self.is_test) if t == test]


NOISE_STREAM = 0x6E6F6973       # 'nois': the generator of the epochs' noise conditions is default_rng([seed, NOISE_STREAM])
VALIDATION_NOISE_SEED = 0x76616C69    # 'vali': the noisy validation sets are rendered once, with this seed
ROOM_STREAM = 0x726F6F6D        # 'room': the generator of the epochs' rooms is default_rng([seed, ROOM_STREAM])
VALIDATION_ROOM_SEED = 0x76726F6D     # 'vrom': the synthetic responses of the reverberant validation sets are built once, from this seed
SMEAR_STREAM = 0x736D6561       # 'smea': the generator of the epochs' spectral resolutions is default_rng([seed, SMEAR_STREAM])
MASKER_STREAM = 0x6D61736B      # 'mask': the generator of the epochs' maskers is default_rng([seed, MASKER_STREAM])
CUTOFF_STREAM = 0x6375746F      # 'cuto': the generator of the epochs' envelope cutoffs is default_rng([seed, CUTOFF_STREAM])
MAX_CUTOFFS = 64                # csrc/f2_internal.h: F2_LOWPASS_MAX_CUTOFFS
RENDER_GROUP = 64               # files per envelope pass, as `prepare input --from-wav`


def draw_epoch_noise(rng, K, B):
    """(level_of (B) int32 in [0, K], noise seed) of one epoch, drawn from rng in that order"""
    level_of = rng.integers(0, K + 1, B).astype(numpy.int32)
    return level_of, int(rng.integers(0, 2 ** 63))


def draw_epoch_rooms(rng, Kr, B):
    """(room_of (B) int32 in [0, Kr], room seed) of one epoch, drawn from rng in that order; Kr is the dry one"""
    room_of = rng.integers(0, Kr + 1, B).astype(numpy.int32)
    return room_of, int(rng.integers(0, 2 ** 63))


def draw_epoch_smear(rng, Km, B):
    """mix_of (B) int32 in [0, Km] of one epoch, drawn from rng; Km is the sharp one (the mixing is deterministic: no seed)"""
    return rng.integers(0, Km + 1, B).astype(numpy.int32)


def draw_epoch_maskers(rng, Kk, B):
    """(masker_level_of (B) int32 in [0, Kk], masker seed) of one epoch, drawn from rng in that order; Kk is the one without a masker"""
    masker_level_of = rng.integers(0, Kk + 1, B).astype(numpy.int32)
    return masker_level_of, int(rng.integers(0, 2 ** 63))


def draw_epoch_cutoffs(rng, Kc, B):
    """cutoff_of (B) int32 in [0, Kc] of one epoch, drawn from rng; Kc is the unfiltered one (the filter is deterministic: no seed)"""
    return rng.integers(0, Kc + 1, B).astype(numpy.int32)


def check_cutoffs(cutoffs):
    """The envelope cutoffs (Hz) of a training run as a tuple of floats, by the rules of f2_lowpass_levels: at most MAX_CUTOFFS,
    every one finite and inside (0, 8000); ValueError otherwise"""
    cutoffs = tuple(float(v) for v in cutoffs)
    if len(cutoffs) > MAX_CUTOFFS:
        raise ValueError("{} envelope cutoffs (at most {})".format(len(cutoffs), MAX_CUTOFFS))
    for v in cutoffs:
        if not (numpy.isfinite(v) and 0.0 < v < 8000.0):
            raise ValueError("envelope cutoff {:g} Hz outside (0, 8000)".format(v))
    return cutoffs


def build_smear_levels(spreads, bands, centre_freqs):
    """((Km, C, C) float64 matrices, names) of the spectral resolutions of a training run, ordered and named as
    Evaluating.EvaluateSmearSweep orders and names them: the spreads (smear.SmearMatrix on the centre frequencies), then the
    numbers of bands (smear.BandMatrix); (None, []) without either"""
    from ... import smear
    from .Evaluating import SmearLevels
    if not len(spreads) and not len(bands):
        return None, []
    spread, counts, names = SmearLevels(spreads, bands, len(centre_freqs))
    return numpy.stack([smear.SmearMatrix(centre_freqs, v) for v in spread] + [smear.BandMatrix(len(centre_freqs), v) for v in counts]), names


def build_rooms(t60s, measured, framerate, drr_db, room_seed):
    """The responses of one epoch (or of the validation sets): reverb.SyntheticRIR(t60, framerate, drr_db, room_seed, level) per
    reverberation time, level its place in the list, then the measured responses, which do not change"""
    from ... import reverb
    return [reverb.SyntheticRIR(v, framerate, drr_db, room_seed, level) for level, v in enumerate(t60s)] + list(measured)


def _render_windows(ctx, waves, centers, coefs, cfg, LPF, CUTOFF, precision, snrs=(), level=None, seed=0, rirs=(), room=None, firs=None,
                    mix=None, masker=None, cutoff=None):
    """Normalised windows of some files through f2_input_batch_noisy, RENDER_GROUP files per call, every file at snrs[level]
    (level None: clean); with `room`, through f2_input_batch_wet with every file in rirs[room]; with `firs` (a filter per level),
    through f2_input_batch_coloured; with `mix` (a (C, C) matrix), through f2_input_batch_smeared with every file mixed by it; with
    `masker` (recordings, masker_of, masker_snrs, level), through f2_input_batch_masked with every file at that masker level; with
    `cutoff` (cutoffs, level), through f2_input_batch_filtered with the envelopes of every file low-passed at cutoffs[level] (LPF
    must be off)"""
    Cn = coefs.shape[0]
    out = numpy.empty((int(sum(len(c) for c in centers)), cfg.dots_per_input, Cn), numpy.float32)
    row = 0
    for g in range(0, len(waves), RENDER_GROUP):
        ws, cs = waves[g:g + RENDER_GROUP], centers[g:g + RENDER_GROUP]
        f64 = any(w.dtype != numpy.int16 for w in ws)
        flat = numpy.concatenate([w.astype(numpy.float64 if f64 else numpy.int16, copy=False) for w in ws])
        offsets = numpy.concatenate([[0], numpy.cumsum([len(w) for w in ws])]).astype(numpy.int64)
        center_offsets = numpy.concatenate([[0], numpy.cumsum([len(c) for c in cs])]).astype(numpy.int64)
        n = int(center_offsets[-1])
        if n == 0:
            continue
        level_of = None if level is None else numpy.full(len(ws), level, numpy.int32)
        front = (flat, _lib.WAVE_F64 if f64 else _lib.WAVE_I16, offsets, coefs, len(ws), Cn, bool(LPF), float(CUTOFF) if LPF else 0.0,
                 precision, center_offsets, numpy.concatenate(cs), cfg.radius, cfg.step, True)
        rooms = (rirs if room is not None else (), None if room is None else numpy.full(len(ws), room, numpy.int32))
        back = (level_of, g, seed, out[row:row + n], _lib.MEM_HOST)
        if cutoff is not None:
            mk = (None, None, (), None) if masker is None else (masker[0], masker[1], masker[2], numpy.full(len(ws), masker[3], numpy.int32))
            ctx.input_batch_filtered(*front, *rooms, snrs, firs, *back[:3], None if mix is None else mix[None],
                                     None if mix is None else numpy.zeros(len(ws), numpy.int32), *mk, cutoff[0],
                                     numpy.full(len(ws), cutoff[1], numpy.int32), *back[3:])
        elif masker is not None:
            ctx.input_batch_masked(*front, *rooms, snrs, firs, *back[:3], None, None, masker[0], masker[1], masker[2],
                                   numpy.full(len(ws), masker[3], numpy.int32), *back[3:])
        elif mix is not None:
            ctx.input_batch_smeared(*front, *rooms, snrs, firs, *back[:3], mix[None], numpy.zeros(len(ws), numpy.int32), *back[3:])
        elif firs is not None:
            ctx.input_batch_coloured(*front, *rooms, snrs, firs, *back)
        elif room is None:
            ctx.input_batch_noisy(*front, snrs, *back)
        else:
            ctx.input_batch_wet(*front, *rooms, snrs, *back)
        row += n
    return out


def TrainFromWav(labelFile=None, LPF=False, CUTOFF=100, snrs=(), seed=None, ctx=None, verbose=1, on_epoch=None, t60s=(), rirs=(),
                 drr_db=0.0, colours=(), noise_taps=1025, spreads=(), bands=(), maskers=(), masker_snrs=(), cutoffs=()):
    """`cnn train --engine hip --from-wav`: trains on windows rendered on the device from the WAV files of the label CSV.

    The TRAIN files go to the trainer once (Trainer.set_waves); the TEST files become normalised windows once, clean - the
    validation set early stopping watches, by train_network's rule. Without `snrs` the training windows are rendered once, clean,
    and the epochs are those of `cnn train --engine hip`. With `snrs` (dB) every epoch draws, from
    numpy.random.default_rng([seed, NOISE_STREAM]), a level in [0, K] per file (K: clean) and a noise seed (draw_epoch_noise), and
    renders the windows again before its steps; one more validation set per level is rendered once with
    VALIDATION_NOISE_SEED, and the history gains 'val_acc_snr' / 'val_loss_snr' (a list per level, an entry per epoch).
    'last_trained_model_results.json' gains augment = {snrs, seed, noise_seed per epoch}. seed None: one is drawn and recorded.
    With `t60s` (seconds) and / or `rirs` (mono WAV files at the corpus' rate, reverb.LoadRIR) every epoch also draws, from
    numpy.random.default_rng([seed, ROOM_STREAM]), a room in [0, Kr] per TRAIN file (Kr: dry) and a room seed (draw_epoch_rooms),
    builds that epoch's synthetic responses on the host (build_rooms: SyntheticRIR(t60, framerate, drr_db, room seed, level); the
    measured ones are fixed) and renders through Trainer.render_wet: room first, then noise at an SNR of the reverberant signal. The
    noise generator is drawn exactly as without rooms. The TEST files are validated clean, at every SNR, and once per room (dry
    of noise; the responses built once from VALIDATION_ROOM_SEED): the history gains 'val_acc_room' / 'val_loss_room' and augment
    gains t60, rirs, drr and room_seed per epoch. A t60 or a measured response beyond reverb.MAX_TAPS raises reverb.py's
    ValueError before any device work.
    With `colours` (names of noise.COLOURS, 'like:<recording.wav>', 'fir:<taps.npy>'; needs `snrs`) a noise level is a pair
    (colour, SNR): the levels are Evaluating.ColourLevels(colours, snrs), colour-major over the SNRs and at most 64 - the level
    numbers of `cnn noisesweep --colours` - and their filters are built once with noise.FromSpec(spec, framerate, noise_taps),
    before any file is read (a bad colour, a recording at another rate or too many taps raise noise.py's ValueError there).
    Every epoch draws a level per TRAIN file and a noise seed exactly as without colours, with K the number of levels, and
    renders through Trainer.render / render_wet(firs=...); the TEST files are validated clean, once per level
    (f2_input_batch_coloured, VALIDATION_NOISE_SEED) and once per room. 'val_acc_snr' / 'val_loss_snr' hold a list per level and
    augment gains colours (a name per level), level_snr_db and noise_taps. 'white' is the filter [1.0]: colours=('white',) trains
    the weights of `snrs` alone, bit for bit.
    With `spreads` (ERB) and / or `bands` (numbers of vocoder bands) every epoch also draws, from
    numpy.random.default_rng([seed, SMEAR_STREAM]), a spectral resolution in [0, Km] per TRAIN file (Km: sharp; draw_epoch_smear)
    and renders through Trainer.render / render_wet(mixes=..., mix_of=...): the envelopes of the file's windows are mixed across
    their channels before they are normalised (f2_trainer_render_smeared). The levels are those of `cnn smearsweep`, in its order -
    the spreads, then the bands - and their matrices are built once with smear.SmearMatrix / smear.BandMatrix before any file is
    read (a bad spread raises smear.py's ValueError there). The noise and room generators are drawn exactly as without them. The
    TEST files are validated sharp as before and once more per resolution, clean and dry (f2_input_batch_smeared): the history
    gains 'val_acc_smear' / 'val_loss_smear' and augment gains spreads, bands and smear_levels (a name per level).
    With `maskers` (recordings, masker.LoadMasker at the corpus' rate; needs `masker_snrs`) a masker level is a pair (recording,
    SNR): the levels are masker.MaskerLevels(maskers, masker_snrs), masker-major over the SNRs and at most 64 - the level numbers
    of `cnn noisesweep --maskers` - and the recordings are read once, before any other file (a recording at another rate raises
    masker.py's ValueError there). Every epoch also draws, from numpy.random.default_rng([seed, MASKER_STREAM]), a masker level
    in [0, Kk] per TRAIN file (Kk: none) and a masker seed (draw_epoch_maskers) and renders through Trainer.render /
    render_wet(maskers=...): behind the room and before the Gaussian noise a cyclic segment of the recording is mixed in at that
    SNR (f2_trainer_render_masked). The segments are drawn with the epoch's noise seed, or with the masker seed where there is no
    noise. The other generators are drawn exactly as without maskers. The TEST files are also validated once per masker level
    (f2_input_batch_masked, VALIDATION_NOISE_SEED): the history gains 'val_acc_masker' / 'val_loss_masker' and augment gains
    maskers (the files), masker_snrs, masker_levels (a name per level) and masker_seed per epoch.
    With `cutoffs` (Hz; the levels of `cnn lpfsweep`, at most 64, every one inside (0, 8000); not together with LPF) every epoch
    also draws, from numpy.random.default_rng([seed, CUTOFF_STREAM]), an envelope cutoff in [0, Kc] per TRAIN file (Kc: unfiltered;
    draw_epoch_cutoffs) and renders through Trainer.render / render_wet(cutoffs=..., cutoff_of=...): the unfiltered envelopes of the
    file are low-passed at that cutoff before its windows are gathered (f2_trainer_render_filtered). Bad cutoffs raise ValueError
    before any file is read. The other generators are drawn exactly as without cutoffs. The TEST files are validated unfiltered as
    before and once more per cutoff, clean, dry and sharp (f2_input_batch_filtered): the history gains 'val_acc_cutoff' /
    'val_loss_cutoff' and augment gains cutoffs.
    on_epoch(iterations, trainer), if given, is called after each epoch's render, before its steps (for tests and for looking at
    what the network is about to see).
    BATCH_SIZE and EPOCHS come from configF2CNN.conf. Returns (F2CNNModel, history)."""
    from configparser import ConfigParser
    from ...config import F2Config
    from ..processing.EnvelopeExtraction import FFT_PRECISION
    from ..processing.GammatoneFiltering import filterbank_from_config
    config = ConfigParser()
    config.read('configF2CNN.conf')
    batch_size = config.getint('CNN', 'BATCH_SIZE', fallback=32)
    epochs = config.getint('CNN', 'EPOCHS', fallback=20)
    snrs = tuple(float(v) for v in snrs)
    colours = tuple(colours.split(',')) if isinstance(colours, str) else tuple(colours)
    cfg = F2Config()
    # (the colours before anything else: a filter that cannot be built is refused here, with noise.py's message)
    firs, level_names = None, ['{:g} dB'.format(v) for v in snrs]
    level_snrs = snrs               # the SNR of every level: with colours, colour-major over snrs
    if colours:
        from ... import noise
        from .Evaluating import ColourLevels, _level_text
        if not snrs:
            raise ValueError("noise colours need the SNRs they are drawn at (snrs)")
        grid = ColourLevels(colours, snrs)
        built = {}
        for spec, _, _ in grid:
            if spec not in built:
                built[spec] = noise.FromSpec(spec, cfg.framerate, noise_taps)
        firs = [built[spec] for spec, _, _ in grid]
        level_snrs = tuple(v for _, _, v in grid)
        level_names = ['{} {}dB'.format(name, _level_text(v)) for _, name, v in grid]
    K = len(level_snrs)
    # (the maskers likewise: a recording that cannot be used is refused here, with masker.py's message)
    maskers = tuple(maskers.split(',')) if isinstance(maskers, str) else tuple(maskers)
    masker_snrs = tuple(float(v) for v in masker_snrs)
    recordings, masker_of, masker_level_snrs, masker_names = None, None, (), []
    if maskers:
        from ... import masker as _masker
        from .Evaluating import _level_text
        if not masker_snrs:
            raise ValueError("maskers need the SNRs they are mixed in at (masker_snrs)")
        masker_grid = _masker.MaskerLevels(maskers, masker_snrs)
        recordings = [_masker.LoadMasker(m, cfg.framerate) for m in maskers]
        masker_of = numpy.array([r for r, _, _ in masker_grid], numpy.int32)
        masker_level_snrs = tuple(v for _, _, v in masker_grid)
        masker_names = ['{} {}dB'.format(name, _level_text(v)) for _, name, v in masker_grid]
    Kk = len(masker_names)
    # (the envelope cutoffs likewise)
    cutoffs = check_cutoffs(cutoffs)
    Kc = len(cutoffs)
    if Kc and LPF:
        raise ValueError("envelope cutoffs per file (cutoffs) and LPF exclude each other: the cutoffs filter unfiltered envelopes")
    cutoff_names = ['{:g} Hz'.format(v) for v in cutoffs]
    # (the mixing matrices likewise: a bad spread or number of bands is refused here, with smear.py's message)
    spreads, bands = tuple(float(v) for v in spreads), tuple(bands)
    centre_freqs, coefs = filterbank_from_config(cfg)
    mixes, smear_names = build_smear_levels(spreads, bands, centre_freqs)
    Km = len(smear_names)
    t60s, rir_files = tuple(float(v) for v in t60s), tuple(rirs)
    Kr = len(t60s) + len(rir_files)
    if seed is None:
        seed = int(numpy.random.default_rng().integers(0, 2 ** 63))
    labelPath = labelFile or os.path.join('trainingData', 'label_data.csv')
    # (the rooms before any file: a response that is too long is refused here, with reverb.py's message)
    from ... import reverb
    measured = [reverb.LoadRIR(r, cfg.framerate) for r in rir_files]
    val_rooms = build_rooms(t60s, measured, cfg.framerate, drr_db, VALIDATION_ROOM_SEED)
    lw = LabelledWaves(labelPath)
    waves = lw.read(cfg.radius * cfg.step)
    train, test = lw.split(False), lw.split(True)
    y_train = numpy.concatenate([lw.signs[k] for k in train]) if train else numpy.zeros(0, numpy.uint8)
    y_test = numpy.concatenate([lw.signs[k] for k in test]) if test else numpy.zeros(0, numpy.uint8)
    if not len(y_train):
        raise ValueError("{} has no TRAIN rows".format(labelPath))
    print('Rising test:', int((y_test == 1).sum()))
    print('Falling test:', int((y_test == 0).sum()))
    print('Rising train:', int((y_train == 1).sum()))
    print('Falling train:', int((y_train == 0).sum()))
    print(len(train), 'train files,', len(test), 'test files; noise levels (dB):', list(snrs) or 'none')
    if colours:
        print('noise colours:', ', '.join(level_names), '| taps', int(noise_taps))
    if Kr:
        print('rooms: t60 (s)', list(t60s) or 'none', '| measured', list(rir_files) or 'none', '| drr (dB) {:g}'.format(float(drr_db)))
    if Km:
        print('spectral resolutions:', ', '.join(smear_names))
    if Kk:
        print('maskers:', ', '.join(masker_names))
    if Kc:
        print('envelope cutoffs:', ', '.join(cutoff_names))
    coefs = numpy.ascontiguousarray(coefs, dtype=numpy.float64)
    ctx = ctx or _lib.default_context()
    try:
        # validation windows: the clean set, then one set per level, in one array with the level as the group
        val = [_render_windows(ctx, [waves[k] for k in test], [lw.centers[k] for k in test], coefs, cfg, LPF, CUTOFF, FFT_PRECISION)]
        for l in range(K if len(y_test) else 0):
            val.append(_render_windows(ctx, [waves[k] for k in test], [lw.centers[k] for k in test], coefs, cfg, LPF, CUTOFF,
                                       FFT_PRECISION, level_snrs, l, VALIDATION_NOISE_SEED, firs=firs))
        for r in range(Kr if len(y_test) else 0):
            val.append(_render_windows(ctx, [waves[k] for k in test], [lw.centers[k] for k in test], coefs, cfg, LPF, CUTOFF,
                                       FFT_PRECISION, rirs=val_rooms, room=r))
        for m in range(Km if len(y_test) else 0):
            val.append(_render_windows(ctx, [waves[k] for k in test], [lw.centers[k] for k in test], coefs, cfg, LPF, CUTOFF,
                                       FFT_PRECISION, mix=mixes[m]))
        for k in range(Kk if len(y_test) else 0):
            val.append(_render_windows(ctx, [waves[j] for j in test], [lw.centers[j] for j in test], coefs, cfg, LPF, CUTOFF,
                                       FFT_PRECISION, seed=VALIDATION_NOISE_SEED, masker=(recordings, masker_of, masker_level_snrs, k)))
        for c in range(Kc if len(y_test) else 0):
            val.append(_render_windows(ctx, [waves[j] for j in test], [lw.centers[j] for j in test], coefs, cfg, LPF, CUTOFF,
                                       FFT_PRECISION, cutoff=(cutoffs, c)))
        x_val, y_val = numpy.concatenate(val), numpy.tile(y_test, len(val))
        groups = numpy.repeat(numpy.arange(len(val), dtype=numpy.int32), len(y_test))
        trainer, rng = _hip_trainer(cfg.dots_per_input, coefs.shape[0], seed, 1e-4, 1e-6, ctx)
        trainer.set_waves([waves[k] for k in train], [lw.centers[k] for k in train], [lw.signs[k] for k in train], coefs, cfg.radius,
                          cfg.step, lpf=bool(LPF), cutoff=float(CUTOFF) if LPF else 0.0, precision=FFT_PRECISION, group=RENDER_GROUP)
        noise_rng = numpy.random.default_rng([seed, NOISE_STREAM])
        room_rng = numpy.random.default_rng([seed, ROOM_STREAM])
        noise_seeds, val_snr = [], {"val_acc_snr": [[] for _ in level_snrs], "val_loss_snr": [[] for _ in level_snrs]}
        room_seeds, val_room = [], {"val_acc_room": [[] for _ in range(Kr)], "val_loss_room": [[] for _ in range(Kr)]}
        smear_rng = numpy.random.default_rng([seed, SMEAR_STREAM])
        val_smear = {"val_acc_smear": [[] for _ in range(Km)], "val_loss_smear": [[] for _ in range(Km)]}
        masker_rng = numpy.random.default_rng([seed, MASKER_STREAM])
        masker_seeds, val_masker = [], {"val_acc_masker": [[] for _ in range(Kk)], "val_loss_masker": [[] for _ in range(Kk)]}
        cutoff_rng = numpy.random.default_rng([seed, CUTOFF_STREAM])
        val_cutoff = {"val_acc_cutoff": [[] for _ in range(Kc)], "val_loss_cutoff": [[] for _ in range(Kc)]}
        if not K and not Kr and not Km and not Kk and not Kc:
            trainer.render()

        def run_epoch():
            level_of, noise_seed = None, 0
            mix_of = draw_epoch_smear(smear_rng, Km, len(train)) if Km else None
            if K:
                level_of, noise_seed = draw_epoch_noise(noise_rng, K, len(train))
                noise_seeds.append(noise_seed)
            masking = {}                                       # (only when asked for: the render without maskers is the one it was)
            if Kk:
                masker_level_of, masker_seed = draw_epoch_maskers(masker_rng, Kk, len(train))
                masker_seeds.append(masker_seed)
                masking = dict(maskers=recordings, masker_of=masker_of, masker_snrs=masker_level_snrs, masker_level_of=masker_level_of)
                if not K:                                      # (the one seed of a render draws the segments too)
                    noise_seed = masker_seed
            if Kc:                                             # (likewise only when asked for)
                masking.update(cutoffs=cutoffs, cutoff_of=draw_epoch_cutoffs(cutoff_rng, Kc, len(train)))
            if Kr:
                room_of, room_seed = draw_epoch_rooms(room_rng, Kr, len(train))
                room_seeds.append(room_seed)
                trainer.render_wet(build_rooms(t60s, measured, cfg.framerate, drr_db, room_seed), room_of, level_snrs, level_of, noise_seed,
                                   firs=firs, mixes=mixes, mix_of=mix_of, **masking)
            elif K or Km or Kk or Kc:
                trainer.render(level_snrs, level_of, noise_seed, firs=firs, mixes=mixes, mix_of=mix_of, **masking)
            if on_epoch:
                on_epoch(trainer.iterations, trainer)
            return trainer.steps(rng.permutation(len(y_train)), batch_size)

        def validate():
            if not len(y_test):
                for per in (val_snr, val_room, val_smear, val_masker, val_cutoff):
                    for k in per:
                        for per_level in per[k]:
                            per_level.append(float("nan"))
                return float("nan"), float("nan")
            _, _, counts, loss_sum = _hip_validate(trainer, ctx, x_val, y_val, groups=groups, n_groups=len(val))
            acc = (counts[:, 0, 0] + counts[:, 1, 1]) / float(len(y_test))
            loss = loss_sum / float(len(y_test))
            for l in range(K):
                val_snr["val_acc_snr"][l].append(float(acc[l + 1]))
                val_snr["val_loss_snr"][l].append(float(loss[l + 1]))
            for r in range(Kr):
                val_room["val_acc_room"][r].append(float(acc[K + 1 + r]))
                val_room["val_loss_room"][r].append(float(loss[K + 1 + r]))
            for m in range(Km):
                val_smear["val_acc_smear"][m].append(float(acc[K + Kr + 1 + m]))
                val_smear["val_loss_smear"][m].append(float(loss[K + Kr + 1 + m]))
            for k in range(Kk):
                val_masker["val_acc_masker"][k].append(float(acc[K + Kr + Km + 1 + k]))
                val_masker["val_loss_masker"][k].append(float(loss[K + Kr + Km + 1 + k]))
            for c in range(Kc):
                val_cutoff["val_acc_cutoff"][c].append(float(acc[K + Kr + Km + Kk + 1 + c]))
                val_cutoff["val_loss_cutoff"][c].append(float(loss[K + Kr + Km + Kk + 1 + c]))
            if verbose and (K or Kr or Km or Kk or Kc):
                print("    val_acc clean {:.4f}".format(acc[0]) + "".join(" | {} {:.4f}".format(s, a) for s, a in zip(level_names, acc[1:])) +
                      "".join(" | room {} {:.4f}".format(r, a) for r, a in enumerate(acc[K + 1:K + Kr + 1])) +
                      "".join(" | {} {:.4f}".format(s, a) for s, a in zip(smear_names, acc[K + Kr + 1:])) +
                      "".join(" | {} {:.4f}".format(s, a) for s, a in zip(masker_names, acc[K + Kr + Km + 1:])) +
                      "".join(" | lpf {} {:.4f}".format(s, a) for s, a in zip(cutoff_names, acc[K + Kr + Km + Kk + 1:])))
            return float(loss[0]), float(acc[0])

        model, history = fit_epochs(run_epoch, validate, trainer.model, len(y_train), epochs, verbose)
    except _lib.F2Error as e:
        if e.code == _lib.F2_ERR_NONPOSITIVE:
            raise ValueError("values must all be positive")
        raise
    if K:
        history.update(val_snr)
    if Kr:
        history.update(val_room)
    if Km:
        history.update(val_smear)
    if Kk:
        history.update(val_masker)
    if Kc:
        history.update(val_cutoff)
    model.save('last_trained_model')
    print("Model saved as 'last_trained_model'.")
    if len(y_test):
        print('Test loss:', history["val_loss"][-1])
        print('Test accuracy:', history["val_acc"][-1])
    results = dict(history)
    if K or Kr or Km or Kk or Kc:
        results["augment"] = {"snrs": list(snrs), "seed": int(seed), "noise_seed": noise_seeds}
    if colours:
        results["augment"].update({"colours": [name for _, name, _ in grid], "level_snr_db": list(level_snrs), "noise_taps": int(noise_taps)})
    if Kr:
        results["augment"].update({"t60": list(t60s), "rirs": list(rir_files), "drr": float(drr_db), "room_seed": room_seeds})
    if Km:
        results["augment"].update({"spreads": list(spreads), "bands": [int(v) for v in bands], "smear_levels": list(smear_names)})
    if Kk:
        results["augment"].update({"maskers": list(maskers), "masker_snrs": list(masker_snrs), "masker_levels": list(masker_names),
                                   "masker_seed": masker_seeds})
    if Kc:
        results["augment"].update({"cutoffs": list(cutoffs)})
    with open('last_trained_model_results.json', 'w') as fp:
        json.dump(results, fp)
    print("History saved as 'last_trained_model_results.json'")
    return model, history


def TrainAndPlotLoss(labelFile=None, inputFile=None, device=None, seed=None, engine="torch"):
    """Trains the CNN on an input tensor (N x 11 x 128, ``prepare input``) and its label CSV (``prepare label``), with
    PyTorch-ROCm autograd (engine 'torch') or the library's own training step (engine 'hip');
    BATCH_SIZE and EPOCHS come from configF2CNN.conf. Saves the weights as 'last_trained_model' (the .npz container
    ``cnn eval`` loads) and the per-epoch history as 'last_trained_model_results.json' (the reference plots it)."""
    from configparser import ConfigParser
    config = ConfigParser()
    config.read('configF2CNN.conf')
    batch_size = config.getint('CNN', 'BATCH_SIZE', fallback=32)
    epochs = config.getint('CNN', 'EPOCHS', fallback=20)
    inputPath = inputFile or os.path.join('trainingData', 'last_input_data.npy')
    labelPath = labelFile or os.path.join('trainingData', 'label_data.csv')
    x_test, y_test, x_train, y_train = SeparateTestTrain(inputPath, labelPath)
    x_train = normalizeInputBatch(x_train)
    x_test = normalizeInputBatch(x_test) if len(x_test) else numpy.empty((0,) + x_train.shape[1:], numpy.float32)
    print('Rising test:', int((y_test == 1).sum()))
    print('Falling test:', int((y_test == 0).sum()))
    print('Rising train:', int((y_train == 1).sum()))
    print('Falling train:', int((y_train == 0).sum()))
    print(x_train.shape, 'train samples')
    print(x_test.shape, 'test samples')
    print("Categories: [falling, rising]")
    model, history = train_network(x_train, y_train, x_test, y_test, batch_size, epochs, device=device, seed=seed, engine=engine)
    model.save('last_trained_model')
    print("Model saved as 'last_trained_model'.")
    # model.evaluate on the test set, through the HIP forward pass that `cnn eval` uses
    if len(x_test):
        scores, labels = model.predict_labels(x_test)
        p = numpy.clip(scores[numpy.arange(len(y_test)), y_test].astype(numpy.float64), 1e-7, 1.0)
        print('Test loss:', float(-numpy.log(p).mean()))
        print('Test accuracy:', float((labels == y_test).mean()))
    with open('last_trained_model_results.json', 'w') as fp:
        json.dump(history, fp)
    print("History saved as 'last_trained_model_results.json'")
    return model, history


MAX_TEST_GROUPS = 1024      # f2_cnn_score_windows tallies up to this many groups
TEST_BY = ("set", "region", "speaker", "phoneme")
TEST_ROWS = ("test", "train", "all")


def GroupLabelRows(csv_rows, by=None, rows='test'):
    """The rows of a label CSV (lists of strings, columns LabelDataGenerator.CSV_COLUMNS) that `cnn test` scores, and their
    groups. rows = 'test' keeps the rows whose first column is 'TEST', 'train' the others (SeparateTestTrain's split), 'all'
    every row. Returns (index, signs, group_ids, names): index (int64) = the kept rows' positions, which are also their rows
    in input_data.npy; signs (uint8) their last column; names = the sorted distinct values of column `by` among the kept rows
    and group_ids (int32) each kept row's position in names - by = None: one group 'all'. No device call in here."""
    from ..processing.LabelDataGenerator import CSV_COLUMNS
    if rows not in TEST_ROWS:
        raise ValueError("rows must be one of {}, not {!r}".format(TEST_ROWS, rows))
    if by is not None and by not in TEST_BY:
        raise ValueError("by must be one of {}, not {!r}".format(TEST_BY, by))
    set_col, sign_col = CSV_COLUMNS.index('set'), CSV_COLUMNS.index('sign')
    index, signs, keys = [], [], []
    for i, row in enumerate(csv_rows):
        is_test = row[set_col] == 'TEST'
        if rows == 'all' or is_test == (rows == 'test'):
            sign = int(row[sign_col])
            if sign not in (0, 1):
                raise ValueError("row {}: sign {!r} is neither 0 nor 1".format(i, row[sign_col]))
            index.append(i)
            signs.append(sign)
            keys.append('all' if by is None else row[CSV_COLUMNS.index(by)])
    names = sorted(set(keys))
    if len(names) > MAX_TEST_GROUPS:
        raise ValueError("column '{}' has {} distinct values among the selected rows; at most {} groups can be tallied"
                         .format(by, len(names), MAX_TEST_GROUPS))
    if not names:
        names = ['all'] if by is None else []
    where = {name: g for g, name in enumerate(names)}
    return (numpy.array(index, numpy.int64), numpy.array(signs, numpy.uint8),
            numpy.array([where[k] for k in keys], numpy.int32), names)


def TestResultPath(model):
    """Where TestModel writes its numbers: '<model>_test.json' next to the model file, a trailing '.npz' of the name dropped
    ('weights.npz' -> 'weights_test.json', as F2CNNModel.load finds 'weights.npz' under 'weights'). None for a model that is
    not a file name: an F2CNNModel object has no place of its own, and nothing is written."""
    if not isinstance(model, str):
        return None
    return (model[:-len('.npz')] if model.endswith('.npz') else model) + '_test.json'


def TestModel(labelFile=None, inputFile=None, model='last_trained_model', by=None, rows='test', ctx=None):
    """`cnn test`: scores a saved model on the labelled windows of `prepare input` / `prepare label` without retraining -
    keras model.evaluate (Training.py:136) - with a breakdown by the CSV column `by` ('set', 'region', 'speaker', 'phoneme').
    The selected rows of the .npy (memory-mapped: only they are copied) go through one f2_cnn_score_windows call, which
    normalises them on the device as normalizeInputBatch does. Prints one line per group and the reference's 'Test loss:' /
    'Test accuracy:' lines for the total and returns the same numbers as a dict. `model` is a file name (written too:
    TestResultPath(model), '<model>_test.json') or an F2CNNModel object (nothing is written)."""
    from ...model import F2CNNModel
    inputPath = inputFile or os.path.join('trainingData', 'last_input_data.npy')
    labelPath = labelFile or os.path.join('trainingData', 'label_data.csv')
    with open(labelPath, 'r') as labels:
        csv_rows = [row for row in csv.reader(labels) if row]
    index, signs, group_ids, names = GroupLabelRows(csv_rows, by, rows)
    data = numpy.load(inputPath, mmap_mode='r')
    if len(index) and index[-1] >= len(data):
        raise ValueError("{} has {} windows, {} has {} rows".format(inputPath, len(data), labelPath, len(csv_rows)))
    x = numpy.ascontiguousarray(data[index], dtype=numpy.float32) if len(index) else numpy.empty((0,) + data.shape[1:], numpy.float32)
    net = model if isinstance(model, F2CNNModel) else F2CNNModel.load(model)
    G = max(len(names), 1)
    try:
        loss, acc, counts, loss_sum = net.evaluate(x, signs, groups=group_ids, n_groups=G, normalize=True, ctx=ctx)
    except _lib.F2Error as e:
        if e.code == _lib.F2_ERR_NONPOSITIVE:
            raise ValueError("values must all be positive")
        raise
    result = {"model": model if isinstance(model, str) else None, "input": inputPath, "label": labelPath, "rows": rows, "by": by,
              "windows": int(len(index)), "loss": loss, "accuracy": acc, "groups": []}
    print("{:<12} {:>9} {:>10} {:>9}   [falling->falling falling->rising | rising->falling rising->rising]".format(
        by or 'group', 'windows', 'loss', 'accuracy'))
    for g, name in enumerate(names):
        c = counts[g]
        n_g = int(c.sum())
        entry = {"name": name, "windows": n_g, "loss": float(loss_sum[g]) / n_g if n_g else None,
                 "accuracy": float(c[0, 0] + c[1, 1]) / n_g if n_g else None, "counts": c.tolist(), "loss_sum": float(loss_sum[g])}
        result["groups"].append(entry)
        print("{:<12} {:>9} {:>10} {:>9}   [{} {} | {} {}]".format(
            name, n_g, "-" if not n_g else "{:.4f}".format(entry["loss"]), "-" if not n_g else "{:.4f}".format(entry["accuracy"]),
            int(c[0, 0]), int(c[0, 1]), int(c[1, 0]), int(c[1, 1])))
    print('Test loss:', loss)
    print('Test accuracy:', acc)
    out = TestResultPath(model)
    if out is not None:
        with open(out, 'w') as fp:
            json.dump(result, fp)
        print("Results saved as '{}'".format(out))
    return result
