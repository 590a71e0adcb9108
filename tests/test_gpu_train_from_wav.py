"""`cnn train --engine hip --from-wav [--augment-snrs ...]` on the labelled WAV corpus of tests/wav_corpus.py: 16 TRAIN and 6 TEST
files at the default configuration (windows of 11 x 128, reach 800), 6 epochs at batch 16.

No accuracy is asserted: nobody has measured what this task gives, with either engine, so the accuracies are printed and the
assertions are about the run - its status, its files, the shape of its history, a falling training loss and the same history from
the same seed."""
import json
import os

import numpy as np
import pytest

import wav_corpus
from f2cnn_amd import cli, config
from f2cnn_amd.model import load_model
from f2cnn_amd.scripts.CNN import Training

pytestmark = pytest.mark.gpu

EPOCHS = 6
KEYS = ("loss", "acc", "val_loss", "val_acc")


@pytest.fixture()
def corpus(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    config.write_default(batch_size=16, epochs=EPOCHS)
    return wav_corpus.write()


def read_history():
    with open("last_trained_model_results.json") as f:
        return json.load(f)


def test_cnn_train_from_wav(corpus, capsys):
    assert cli.main(["cnn", "train", "--engine", "hip", "--from-wav", "--seed", "3"]) == 0
    out = capsys.readouterr().out
    assert "Test accuracy:" in out and not os.path.exists("trainingData/last_input_data.npy")
    model = load_model("last_trained_model")
    assert (model.rows, model.channels) == (11, 128)
    h = read_history()
    assert set(h) == set(KEYS) and len({len(h[k]) for k in KEYS}) == 1 and 1 <= len(h["loss"]) <= EPOCHS
    print("from-wav history", h)
    assert len(h["loss"]) >= 2 and h["loss"][-1] < h["loss"][0]
    assert cli.main(["cnn", "train", "--engine", "hip", "--from-wav", "--seed", "3"]) == 0
    assert read_history() == h


def test_cnn_train_from_wav_with_noise(corpus, capsys):
    argv = ["cnn", "train", "--engine", "hip", "--from-wav", "--augment-snrs", "20,3", "--seed", "3", "--lpf", "50"]
    assert cli.main(argv) == 0
    assert "val_acc clean" in capsys.readouterr().out
    h = read_history()
    n = len(h["loss"])
    assert set(h) == set(KEYS) | {"val_acc_snr", "val_loss_snr", "augment"} and all(len(h[k]) == n for k in KEYS) and n >= 2
    assert len(h["val_acc_snr"]) == len(h["val_loss_snr"]) == 2
    assert all(len(per_level) == n for k in ("val_acc_snr", "val_loss_snr") for per_level in h[k])
    assert h["augment"]["snrs"] == [20.0, 3.0] and h["augment"]["seed"] == 3 and len(h["augment"]["noise_seed"]) == n
    assert len(set(h["augment"]["noise_seed"])) == n
    print("augmented history", h)
    assert h["loss"][-1] < h["loss"][0]
    load_model("last_trained_model")
    assert cli.main(argv) == 0
    assert read_history() == h


def test_every_epoch_sees_other_windows(corpus):
    """TrainFromWav's on_epoch hook: the rendered set before the steps of epochs 0 and 1. With levels drawn per file and a new noise
    seed per epoch the two differ; without --augment-snrs they are the same bytes, rendered once."""
    seen = []
    Training.TrainFromWav(snrs=(20.0, 3.0), seed=3, verbose=0, on_epoch=lambda it, t: seen.append(t.windows()) if len(seen) < 2 else None)
    (x0, y0), (x1, y1) = seen
    assert x0.shape == x1.shape == (16 * wav_corpus.SEGMENTS, 11, 128) and np.array_equal(y0, y1)
    assert np.isfinite(x0).all() and x0.min() == 0.0 and x0.max() == 1.0
    assert not np.array_equal(x0, x1)
    # labels in sorted file order, each file's rows in CSV order
    want = np.concatenate([corpus[k][2] for k in sorted(k for k in corpus if k.startswith("TRAIN"))])
    assert np.array_equal(y0, want)
    seen.clear()
    Training.TrainFromWav(seed=3, verbose=0, on_epoch=lambda it, t: seen.append(t.windows()) if len(seen) < 2 else None)
    assert np.array_equal(seen[0][0], seen[1][0])
