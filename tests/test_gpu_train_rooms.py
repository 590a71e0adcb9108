"""Training in rooms: Trainer.render_wet against f2_input_batch_wet group by group and against render, and `cnn train --engine hip
--from-wav --augment-t60 ... --augment-snrs ...` on a labelled WAV corpus written into the test's own directory
(tests/wav_corpus.py: 6 TRAIN and 2 TEST files of 1 s at the default configuration, windows of 11 x 128), two epochs at batch 16.
No accuracy is asserted, as in tests/test_gpu_train_from_wav.py: the assertions are about the run, its files and its repeatability."""
import json

import numpy as np
import pytest

import noisy_batch as nb
import train_referee as tr
import wav_corpus
from f2cnn_amd import _lib, cli, config
from f2cnn_amd.model import F2CNNModel, load_model
from f2cnn_amd.reverb import SyntheticRIR
from f2cnn_amd.scripts.CNN import Training
from f2cnn_amd.trainer import Trainer
from noisy_batch import B, C, K, LEVEL_OF, R, RADIUS, SEED, SNR, STEP, bits

pytestmark = pytest.mark.gpu

RIRS = [SyntheticRIR(1.0, t, seed=9, level=l) for l, t in enumerate((7, 1025, 2500))]     # (one tap would be the unit response)
KR = len(RIRS)
ROOM_OF = (1, 3, 0, 2, 0, 1)          # tests/noisy_batch.py's six utterances: every room and the dry one
EPOCHS, N_TRAIN, N_TEST = 2, 6, 2
KEYS = ("loss", "acc", "val_loss", "val_acc")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    with c.options(spectral_min_rows=0):        # the 1 s row takes the spectral route in every call of this module
        yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    flat, offsets = nb.waves()
    cs, _ = nb.centers()
    rng = np.random.default_rng(3)
    return [flat[offsets[b]:offsets[b + 1]] for b in range(B)], cs, [rng.integers(0, 2, len(c)).astype(np.uint8) for c in cs]


def new_trainer(ctx):
    return Trainer(F2CNNModel.glorot(7, R, C, zero_bias=False), lr=1e-3, rho=0.9, eps=1e-7, decay=0.5, drop=tr.DROP, seed=5, ctx=ctx)


def test_render_wet_is_input_batch_wet_group_by_group(ctx, corpus):
    waves, cs, signs = corpus
    flat, offsets = nb.waves()
    coefs = nb.coefs()
    room, lev = np.array(ROOM_OF, np.int32), np.array(LEVEL_OF, np.int32)
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, coefs, RADIUS, STEP, lpf=True, cutoff=50.0, group=4)      # groups of 4 and 2 utterances
    t.render_wet(RIRS, room, SNR, lev, SEED)
    x, y = t.windows()
    assert np.array_equal(y, np.concatenate(signs)) and np.isfinite(x).all()
    row = 0
    for g in range(0, B, 4):
        e = min(g + 4, B)
        part = flat[int(offsets[g]):int(offsets[e])]
        coff = np.concatenate([[0], np.cumsum([len(c) for c in cs[g:e]])]).astype(np.int64)
        want = np.full((int(coff[-1]), R, C), np.nan, np.float32)
        ctx.input_batch_wet(part, _lib.WAVE_I16, offsets[g:e + 1] - offsets[g], coefs, e - g, C, True, 50.0, _lib.FFT_F32, coff,
                            np.concatenate(cs[g:e]), RADIUS, STEP, True, RIRS, room[g:e], SNR, lev[g:e], g, SEED, want, _lib.MEM_HOST)
        assert bits(x[row:row + len(want)]).tobytes() == bits(want).tobytes(), g
        row += len(want)
    assert row == len(x)
    # a second render: the same bytes; a bad room: an error that names the utterance and changes nothing
    t.render_wet(RIRS, room, SNR, lev, SEED)
    assert bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    bad = room.copy()
    bad[5] = KR + 1
    with pytest.raises(_lib.F2Error, match="utterance 5") as ei:
        t.render_wet(RIRS, bad, SNR, lev, SEED)
    assert ei.value.code == _lib.F2_ERR_INVALID and bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    t.close()


def test_render_wet_without_rooms_is_render(ctx, corpus):
    waves, cs, signs = corpus
    coff = np.concatenate([[0], np.cumsum([len(c) for c in cs])])
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, nb.coefs(), RADIUS, STEP, group=4)
    t.render(SNR, LEVEL_OF, SEED)
    noisy, _ = t.windows()
    t.render()
    clean, _ = t.windows()
    for kw in (dict(), dict(rirs=RIRS), dict(room_of=(0,) * B)):
        t.render_wet(snrs=SNR, level_of=LEVEL_OF, seed=SEED, **kw)
        assert bits(t.windows()[0]).tobytes() == bits(noisy).tobytes(), kw.keys()
    t.render_wet()
    assert bits(t.windows()[0]).tobytes() == bits(clean).tobytes()
    # rooms and no noise: an utterance in the dry room has the clean render's windows (the same samples, as float64), the others not
    t.render_wet(RIRS, ROOM_OF)
    wet, _ = t.windows()
    t.close()
    for u, l in enumerate(ROOM_OF):
        s = slice(int(coff[u]), int(coff[u + 1]))
        if s.stop > s.start:
            assert np.array_equal(wet[s], clean[s]) == (l == KR), u


@pytest.fixture()
def wavs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    config.write_default(batch_size=16, epochs=EPOCHS)
    return wav_corpus.write(n_train=N_TRAIN, n_test=N_TEST)


def read_history():
    with open("last_trained_model_results.json") as f:
        return json.load(f)


def test_cnn_train_in_rooms_twice(wavs, capsys):
    argv = ["cnn", "train", "--engine", "hip", "--from-wav", "--augment-t60", "0.05,0.1", "--augment-snrs", "10", "--seed", "1"]
    assert cli.main(argv) == 0
    assert "room 1" in capsys.readouterr().out
    h = read_history()
    weights = load_model("last_trained_model").ordered()
    n = len(h["loss"])
    assert set(h) == set(KEYS) | {"val_acc_snr", "val_loss_snr", "val_acc_room", "val_loss_room", "augment"} and n == EPOCHS
    assert all(len(h[k]) == n for k in KEYS)
    assert len(h["val_acc_room"]) == len(h["val_loss_room"]) == 2 and len(h["val_acc_snr"]) == 1
    assert all(len(per) == n for k in ("val_acc_room", "val_loss_room", "val_acc_snr") for per in h[k])
    a = h["augment"]
    assert a["t60"] == [0.05, 0.1] and a["rirs"] == [] and a["drr"] == 0.0 and a["snrs"] == [10.0] and a["seed"] == 1
    assert len(a["room_seed"]) == len(a["noise_seed"]) == n and len(set(a["room_seed"])) == n
    print("history in rooms", h)
    assert cli.main(argv) == 0
    assert read_history() == h
    for w0, w1 in zip(weights, load_model("last_trained_model").ordered()):
        assert np.asarray(w0).tobytes() == np.asarray(w1).tobytes()


def test_every_epoch_sees_other_rooms(wavs):
    """on_epoch: the rendered set before the steps of epochs 0 and 1. Rooms without noise, so that a file that drew the dry room
    has the clean render's windows; the rooms are redrawn from default_rng([seed, ROOM_STREAM]) as TrainFromWav draws them."""
    seen = []
    Training.TrainFromWav(t60s=(0.05, 0.1), seed=1, verbose=0, on_epoch=lambda it, t: seen.append(t.windows()[0]))
    x0, x1 = seen
    assert x0.shape == x1.shape == (N_TRAIN * wav_corpus.SEGMENTS, 11, 128) and np.isfinite(x0).all()
    assert not np.array_equal(x0, x1)
    seen.clear()
    Training.TrainFromWav(seed=1, verbose=0, on_epoch=lambda it, t: seen.append(t.windows()[0]))
    clean = seen[0]
    rng = np.random.default_rng([1, Training.ROOM_STREAM])
    per = wav_corpus.SEGMENTS
    for x in (x0, x1):
        room_of, _ = Training.draw_epoch_rooms(rng, 2, N_TRAIN)
        for f, l in enumerate(room_of):
            assert np.array_equal(x[f * per:(f + 1) * per], clean[f * per:(f + 1) * per]) == (l == 2), (f, l)
