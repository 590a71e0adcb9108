"""Training under recorded maskers: `cnn train --engine hip --from-wav --augment-maskers ... --augment-masker-snrs ...` on a labelled
WAV corpus written into the test's own directory (tests/wav_corpus.py: 6 TRAIN and 2 TEST files of 1 s at the default configuration,
windows of 11 x 128), two epochs at batch 16, with two short recordings written beside it. No accuracy is asserted, as in
tests/test_gpu_train_smear.py: the assertions are about the run, its files, its repeatability and what every epoch renders."""
import json

import numpy as np
import pytest
from scipy.io import wavfile

import wav_corpus
from f2cnn_amd import _lib, cli, config, masker
from f2cnn_amd.config import F2Config
from f2cnn_amd.model import load_model
from f2cnn_amd.scripts.CNN import Training
from noisy_batch import bits

pytestmark = pytest.mark.gpu

EPOCHS, N_TRAIN, N_TEST = 2, 6, 2
KEYS = ("loss", "acc", "val_loss", "val_acc")
MASKERS, SNRS = ("babble.wav", "cafe.wav"), (10.0, 0.0)


@pytest.fixture()
def wavs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    config.write_default(batch_size=16, epochs=EPOCHS)
    rng = np.random.default_rng(8)
    for name, n in zip(MASKERS, (5000, 23000)):        # one shorter than the files (it wraps), one longer
        envelope = 1.0 + np.sin(2 * np.pi * 4.0 * np.arange(n) / 16000.0)      # a 4 Hz modulation of its own
        wavfile.write(name, 16000, (rng.standard_normal(n) * 2500 * envelope).astype(np.int16))
    return wav_corpus.write(n_train=N_TRAIN, n_test=N_TEST)


def read_history():
    with open("last_trained_model_results.json") as f:
        return json.load(f)


def test_cnn_train_under_maskers_twice(wavs, capsys):
    argv = ["cnn", "train", "--engine", "hip", "--from-wav", "--augment-maskers", ",".join(MASKERS), "--augment-masker-snrs", "10,0", "--seed", "1"]
    assert cli.main(argv) == 0
    assert "babble 10dB" in capsys.readouterr().out
    h = read_history()
    weights = load_model("last_trained_model").ordered()
    n = len(h["loss"])
    assert set(h) == set(KEYS) | {"val_acc_masker", "val_loss_masker", "augment"} and n == EPOCHS
    assert len(h["val_acc_masker"]) == len(h["val_loss_masker"]) == 4 and all(len(per) == n for per in h["val_acc_masker"] + h["val_loss_masker"])
    assert all(np.isfinite(per).all() for per in h["val_loss_masker"])
    a = h["augment"]
    assert a["maskers"] == list(MASKERS) and a["masker_snrs"] == [10.0, 0.0] and a["seed"] == 1 and len(a["masker_seed"]) == n
    assert a["masker_levels"] == ["babble 10dB", "babble 0dB", "cafe 10dB", "cafe 0dB"]
    print("history under maskers", h)
    assert cli.main(argv) == 0
    assert read_history() == h
    for w0, w1 in zip(weights, load_model("last_trained_model").ordered()):
        assert np.asarray(w0).tobytes() == np.asarray(w1).tobytes()


def test_every_epoch_sees_the_drawn_maskers(wavs):
    """on_epoch: the rendered set before the steps of epochs 0 and 1 is one f2_input_batch_masked of the TRAIN files at the levels and
    with the seed redrawn here from default_rng([seed, MASKER_STREAM]); with Gaussian noise beside them the segments follow its seed"""
    from f2cnn_amd.scripts.processing.EnvelopeExtraction import FFT_PRECISION
    from f2cnn_amd.scripts.processing.GammatoneFiltering import filterbank_from_config
    cfg = F2Config()
    _, coefs = filterbank_from_config(cfg)
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    recordings = [masker.LoadMasker(m, cfg.framerate) for m in MASKERS]
    grid = masker.MaskerLevels(MASKERS, SNRS)
    masker_of, level_snrs = [r for r, _, _ in grid], [v for _, _, v in grid]
    lw = Training.LabelledWaves("trainingData/label_data.csv")
    waves = lw.read(cfg.radius * cfg.step)
    train = lw.split(False)
    flat = np.concatenate([waves[k] for k in train])
    offsets = np.concatenate([[0], np.cumsum([len(waves[k]) for k in train])]).astype(np.int64)
    coff = np.concatenate([[0], np.cumsum([len(lw.centers[k]) for k in train])]).astype(np.int64)
    ctx = _lib.default_context()
    for snrs in ((), (20.0,)):
        seen = []
        Training.TrainFromWav(maskers=MASKERS, masker_snrs=SNRS, snrs=snrs, seed=1, verbose=0, on_epoch=lambda it, t: seen.append(t.windows()[0]))
        assert len(seen) == EPOCHS and not np.array_equal(seen[0], seen[1])
        rng = np.random.default_rng([1, Training.MASKER_STREAM])
        noise_rng = np.random.default_rng([1, Training.NOISE_STREAM])
        for x in seen:
            level_of, seed = None, None
            if snrs:
                level_of, seed = Training.draw_epoch_noise(noise_rng, len(snrs), len(train))
            masker_level_of, masker_seed = Training.draw_epoch_maskers(rng, len(grid), len(train))
            want = np.full(x.shape, np.nan, np.float32)
            ctx.input_batch_masked(flat, _lib.WAVE_I16, offsets, coefs, len(train), coefs.shape[0], False, 0.0, FFT_PRECISION, coff,
                                   np.concatenate([lw.centers[k] for k in train]), cfg.radius, cfg.step, True, (), None, snrs, None, level_of, 0,
                                   masker_seed if seed is None else seed, None, None, recordings, masker_of, level_snrs, masker_level_of, want,
                                   _lib.MEM_HOST)
            assert bits(x).tobytes() == bits(want).tobytes()
