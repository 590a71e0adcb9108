"""Training across envelope cutoffs: Trainer.render / render_wet(cutoffs=..., cutoff_of=...) in groups of two over five files against
f2_input_batch_filtered group by group, against the render without the arguments, and TrainFromWav(cutoffs=...) on a labelled WAV
corpus written into the test's own directory (tests/wav_corpus.py: 6 TRAIN and 2 TEST files of 1 s at the default configuration,
windows of 11 x 128), two epochs at batch 16. No accuracy is asserted, as in tests/test_gpu_train_smear.py: the assertions are about
the run, its history and what it leaves unchanged."""
import numpy as np
import pytest

import f2cnn_oracle as orc
import speechlike
import train_referee as tr
import wav_corpus
from f2cnn_amd import _lib, config
from f2cnn_amd.config import F2Config
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.reverb import SyntheticRIR
from f2cnn_amd.scripts.CNN import Training
from f2cnn_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

# the five files of tests/test_gpu_input_batch_filtered.py through the narrowest network with a dense1 input (11 x 10)
C, RADIUS, STEP = 10, 5, 160
R, REACH = 2 * RADIUS + 1, RADIUS * STEP
LENGTHS = (1500, 4097, 9000, 2500, 6001)
NB, GROUP = len(LENGTHS), 2                     # groups of 2, 2 and 1
CUTOFFS = (5.0, 50.0, 400.0)
KC = len(CUTOFFS)
CUTOFF_OF = (1, 0, 2, 3, 1)
SNR, LEVEL_OF, SEED = (20.0, 6.0), (0, 2, 1, 0, 1), 0x1234_5678_9ABC
RIRS = [SyntheticRIR(1.0, t, seed=9, level=l) for l, t in enumerate((7, 1025))]
ROOM_OF = (1, 2, 0, 2, 0)
EPOCHS, N_TRAIN, N_TEST = 2, 6, 2


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def corpus():
    waves = [speechlike.make(470 + i, n)[0].astype(np.int16) for i, n in enumerate(LENGTHS)]
    rng = np.random.default_rng(11)
    cs = []
    for n in LENGTHS:
        c = rng.integers(REACH, n - REACH, size=4) if n >= 2 * REACH + 1 else np.zeros(0, np.int64)
        if len(c):
            c[0], c[-1] = REACH, n - 1 - REACH
        cs.append(c.astype(np.int64))
    signs = [(np.arange(len(c)) % 2).astype(np.uint8) for c in cs]
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))
    return waves, cs, signs, coefs


def new_trainer(ctx):
    return Trainer(F2CNNModel.glorot(7, R, C, zero_bias=False), lr=1e-3, rho=0.9, eps=1e-7, decay=0.5, drop=tr.DROP, seed=5, ctx=ctx)


@pytest.mark.parametrize("stages", ("alone", "rooms and noise"))
def test_render_with_cutoffs_is_input_batch_filtered_group_by_group(ctx, corpus, stages):
    waves, cs, signs, coefs = corpus
    full = stages != "alone"
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    flat = np.concatenate(waves)
    room, lev, cof = np.array(ROOM_OF, np.int32), np.array(LEVEL_OF, np.int32), np.array(CUTOFF_OF, np.int32)
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, coefs, RADIUS, STEP, group=GROUP)

    def render(**kw):
        if full:
            t.render_wet(RIRS, room, SNR, lev, SEED, **kw)
        else:
            t.render(**kw)
    render()
    before = t.windows()[0]
    render(cutoffs=CUTOFFS, cutoff_of=cof)
    x, y = t.windows()
    assert np.array_equal(y, np.concatenate(signs)) and np.isfinite(x).all() and len(x) == 16
    row = 0
    for g in range(0, NB, GROUP):                             # group g starts at first_utterance = g; the last one is partial
        e = min(g + GROUP, NB)
        coff = np.concatenate([[0], np.cumsum([len(c) for c in cs[g:e]])]).astype(np.int64)
        want = np.full((int(coff[-1]), R, C), np.nan, np.float32)
        ctx.input_batch_filtered(flat[int(offsets[g]):int(offsets[e])], _lib.WAVE_I16, offsets[g:e + 1] - offsets[g], coefs, e - g, C, False,
                                 0.0, _lib.FFT_F32, coff, np.concatenate(cs[g:e]), RADIUS, STEP, True, RIRS if full else (),
                                 room[g:e] if full else None, SNR if full else (), None, lev[g:e] if full else None, g, SEED if full else 0,
                                 None, None, None, None, (), None, CUTOFFS, cof[g:e], want, _lib.MEM_HOST)
        assert bits(x[row:row + len(want)]).tobytes() == bits(want).tobytes(), g
        row += len(want)
    assert row == len(x)
    # utterance 3 is unfiltered: its windows are the plain render's; the others are not
    woff = np.concatenate([[0], np.cumsum([len(c) for c in cs])])
    assert bits(x[woff[3]:woff[4]]).tobytes() == bits(before[woff[3]:woff[4]]).tobytes()
    assert not np.array_equal(x[:woff[3]], before[:woff[3]]) and not np.array_equal(x[woff[4]:], before[woff[4]:])
    # without the arguments, with no cutoffs and with every file unfiltered it is the render it was; a second filtered render
    # gives the same bytes; a bad level names its utterance and changes nothing
    for kw in (dict(), dict(cutoffs=(), cutoff_of=None), dict(cutoffs=CUTOFFS, cutoff_of=None), dict(cutoffs=CUTOFFS, cutoff_of=(KC,) * NB)):
        render(**kw)
        assert bits(t.windows()[0]).tobytes() == bits(before).tobytes(), kw
    render(cutoffs=CUTOFFS, cutoff_of=cof)
    assert bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    bad = cof.copy()
    bad[3] = KC + 1
    with pytest.raises(_lib.F2Error, match="utterance 3") as ei:
        render(cutoffs=CUTOFFS, cutoff_of=bad)
    assert ei.value.code == _lib.F2_ERR_INVALID and bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    t.close()


def test_a_trainer_set_with_lpf_refuses_the_stage(ctx, corpus):
    waves, cs, signs, coefs = corpus
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, coefs, RADIUS, STEP, lpf=True, cutoff=50.0, group=GROUP)
    t.render()
    before = t.windows()[0]
    with pytest.raises(_lib.F2Error, match="lpf") as ei:
        t.render(cutoffs=CUTOFFS, cutoff_of=CUTOFF_OF)
    assert ei.value.code == _lib.F2_ERR_INVALID and "cutoff" in str(ei.value)
    assert bits(t.windows()[0]).tobytes() == bits(before).tobytes()
    t.render(cutoffs=CUTOFFS, cutoff_of=None)                 # (no stage: the low-passed render it was)
    assert bits(t.windows()[0]).tobytes() == bits(before).tobytes()
    t.close()


@pytest.fixture()
def wavs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    config.write_default(batch_size=16, epochs=EPOCHS)
    return wav_corpus.write(n_train=N_TRAIN, n_test=N_TEST)


def test_train_from_wav_with_cutoffs(wavs):
    """The history has a list per cutoff with an entry per epoch; on_epoch sees, before the steps of every epoch, one
    f2_input_batch_filtered of the TRAIN files at the levels redrawn here from default_rng([seed, CUTOFF_STREAM]); a file drawn
    filtered differs from the same file unfiltered"""
    from f2cnn_amd.scripts.processing.EnvelopeExtraction import FFT_PRECISION
    from f2cnn_amd.scripts.processing.GammatoneFiltering import filterbank_from_config
    cutoffs = (10.0, 50.0)
    seen = []
    _, h = Training.TrainFromWav(cutoffs=cutoffs, seed=1, verbose=0, on_epoch=lambda it, t: seen.append(t.windows()[0]))
    assert len(h["loss"]) == EPOCHS and len(seen) == EPOCHS
    assert len(h["val_acc_cutoff"]) == len(h["val_loss_cutoff"]) == 2
    assert all(len(per) == EPOCHS and np.isfinite(per).all() for per in h["val_acc_cutoff"] + h["val_loss_cutoff"])
    assert not any(k in h for k in ("val_acc_snr", "val_acc_room", "val_acc_smear", "val_acc_masker"))
    cfg = F2Config()
    _, coefs = filterbank_from_config(cfg)
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    lw = Training.LabelledWaves("trainingData/label_data.csv")
    waves = lw.read(cfg.radius * cfg.step)
    train = lw.split(False)
    flat = np.concatenate([waves[k] for k in train])
    offsets = np.concatenate([[0], np.cumsum([len(waves[k]) for k in train])]).astype(np.int64)
    coff = np.concatenate([[0], np.cumsum([len(lw.centers[k]) for k in train])]).astype(np.int64)
    cen = np.concatenate([lw.centers[k] for k in train])
    ctx = _lib.default_context()

    def windows(cutoff_of):
        want = np.full(seen[0].shape, np.nan, np.float32)
        ctx.input_batch_filtered(flat, _lib.WAVE_I16, offsets, coefs, len(train), coefs.shape[0], False, 0.0, FFT_PRECISION, coff, cen,
                                 cfg.radius, cfg.step, True, (), None, (), None, None, 0, 0, None, None, None, None, (), None, cutoffs,
                                 cutoff_of, want, _lib.MEM_HOST)
        return want
    plain = windows(None)
    rng = np.random.default_rng([1, Training.CUTOFF_STREAM])
    drawn = []
    for x in seen:
        cutoff_of = Training.draw_epoch_cutoffs(rng, 2, len(train))
        drawn.append(cutoff_of)
        assert bits(x).tobytes() == bits(windows(cutoff_of)).tobytes()
        for b, l in enumerate(cutoff_of):                     # a file drawn filtered against the same file unfiltered
            same = bits(x[coff[b]:coff[b + 1]]).tobytes() == bits(plain[coff[b]:coff[b + 1]]).tobytes()
            assert same == (l == 2), (b, l)
    assert not np.array_equal(drawn[0], drawn[1]) and any((d < 2).any() for d in drawn)


def test_without_cutoffs_the_run_is_the_one_it_was(wavs):
    """TrainFromWav(snrs=..., cutoffs=()) against the epoch loop written out with the calls that were there before the cutoffs: the
    noise generator is drawn as before and the weights are the same bytes"""
    from f2cnn_amd.scripts.processing.EnvelopeExtraction import FFT_PRECISION
    from f2cnn_amd.scripts.processing.GammatoneFiltering import filterbank_from_config
    snrs = (20.0, 0.0)
    model, history = Training.TrainFromWav(snrs=snrs, seed=1, verbose=0, cutoffs=())
    assert "val_acc_cutoff" not in history and len(history["loss"]) == EPOCHS
    cfg = F2Config()
    _, coefs = filterbank_from_config(cfg)
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    lw = Training.LabelledWaves("trainingData/label_data.csv")
    waves = lw.read(cfg.radius * cfg.step)
    train = lw.split(False)
    ctx = _lib.default_context()
    trainer, rng = Training._hip_trainer(cfg.dots_per_input, coefs.shape[0], 1, 1e-4, 1e-6, ctx)
    trainer.set_waves([waves[k] for k in train], [lw.centers[k] for k in train], [lw.signs[k] for k in train], coefs, cfg.radius, cfg.step,
                      lpf=False, cutoff=0.0, precision=FFT_PRECISION, group=Training.RENDER_GROUP)
    noise_rng = np.random.default_rng([1, Training.NOISE_STREAM])
    n = sum(len(lw.signs[k]) for k in train)
    for _ in range(EPOCHS):
        level_of, noise_seed = Training.draw_epoch_noise(noise_rng, len(snrs), len(train))
        ctx.trainer_render(trainer.handle, snrs, level_of, noise_seed)       # the entry without any later stage
        trainer.steps(rng.permutation(n), 16)
    old = trainer.model()
    for w0, w1 in zip(old.ordered(), model.ordered()):
        assert np.asarray(w0).tobytes() == np.asarray(w1).tobytes()
    trainer.close()
