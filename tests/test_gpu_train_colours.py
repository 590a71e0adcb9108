"""Training against colours: Trainer.render(firs=...) against f2_input_batch_coloured group by group, against render_wet and render,
and `cnn train --engine hip --from-wav --augment-snrs ... --augment-colours ...` on a labelled WAV corpus written into the test's own
directory (tests/wav_corpus.py: 6 TRAIN and 2 TEST files of 1 s at the default configuration, windows of 11 x 128), two epochs at
batch 16. No accuracy is asserted, as in tests/test_gpu_train_rooms.py: the assertions are about the run, its files and its
repeatability."""
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
from test_gpu_shaped_noise import random_filter

pytestmark = pytest.mark.gpu

FIRS = [random_filter(t, 3) for t in (5, 1025, 2048)]
RIRS = [SyntheticRIR(1.0, t, seed=9, level=l) for l, t in enumerate((7, 1025))]
ROOM_OF = (1, 2, 0, 2, 0, 1)
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


@pytest.mark.parametrize("rooms", (False, True))
def test_render_with_filters_is_input_batch_coloured_group_by_group(ctx, corpus, rooms):
    waves, cs, signs = corpus
    flat, offsets = nb.waves()
    coefs = nb.coefs()
    room, lev = np.array(ROOM_OF, np.int32), np.array(LEVEL_OF, np.int32)
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, coefs, RADIUS, STEP, lpf=True, cutoff=50.0, group=4)      # groups of 4 and 2 utterances
    if rooms:
        t.render_wet(RIRS, room, SNR, lev, SEED, firs=FIRS)
    else:
        t.render(SNR, lev, SEED, firs=FIRS)
    x, y = t.windows()
    assert np.array_equal(y, np.concatenate(signs)) and np.isfinite(x).all()
    row = 0
    for g in range(0, B, 4):                                  # the second group starts at first_utterance = 4
        e = min(g + 4, B)
        part = flat[int(offsets[g]):int(offsets[e])]
        coff = np.concatenate([[0], np.cumsum([len(c) for c in cs[g:e]])]).astype(np.int64)
        want = np.full((int(coff[-1]), R, C), np.nan, np.float32)
        ctx.input_batch_coloured(part, _lib.WAVE_I16, offsets[g:e + 1] - offsets[g], coefs, e - g, C, True, 50.0, _lib.FFT_F32, coff,
                                 np.concatenate(cs[g:e]), RADIUS, STEP, True, RIRS if rooms else (), room[g:e] if rooms else None, SNR, FIRS,
                                 lev[g:e], g, SEED, want, _lib.MEM_HOST)
        assert bits(x[row:row + len(want)]).tobytes() == bits(want).tobytes(), g
        row += len(want)
    assert row == len(x)
    # a second render: the same bytes; a bad filter: an error that names the level and changes nothing
    (t.render_wet(RIRS, room, SNR, lev, SEED, firs=FIRS) if rooms else t.render(SNR, lev, SEED, firs=FIRS))
    assert bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    bad = [FIRS[0], FIRS[1] * np.nan, FIRS[2]]
    with pytest.raises(_lib.F2Error, match="level 1") as ei:
        t.render(SNR, lev, SEED, firs=bad)
    assert ei.value.code == _lib.F2_ERR_INVALID and bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    t.close()


def test_without_filters_and_with_white_filters_it_is_the_render_it_was(ctx, corpus):
    waves, cs, signs = corpus
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, nb.coefs(), RADIUS, STEP, group=4)
    t.render_wet(RIRS, ROOM_OF, SNR, LEVEL_OF, SEED)
    wet, _ = t.windows()
    t.render(SNR, LEVEL_OF, SEED)
    noisy, _ = t.windows()
    assert not np.array_equal(wet, noisy)
    # firs=None is render_wet, through the coloured entry too
    t.render_wet(RIRS, ROOM_OF, SNR, LEVEL_OF, SEED, firs=None)
    assert bits(t.windows()[0]).tobytes() == bits(wet).tobytes()
    ctx.trainer_render_coloured(t.handle, RIRS, ROOM_OF, SNR, None, LEVEL_OF, SEED)
    assert bits(t.windows()[0]).tobytes() == bits(wet).tobytes()
    # white filters are render
    t.render(SNR, LEVEL_OF, SEED, firs=[np.ones(1)] * K)
    assert bits(t.windows()[0]).tobytes() == bits(noisy).tobytes()
    t.render_wet(RIRS, ROOM_OF, SNR, LEVEL_OF, SEED, firs=[np.ones(1)] * K)
    assert bits(t.windows()[0]).tobytes() == bits(wet).tobytes()
    # ... and colours are not
    t.render(SNR, LEVEL_OF, SEED, firs=FIRS)
    assert not np.array_equal(t.windows()[0], noisy)
    t.close()


@pytest.fixture()
def wavs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    config.write_default(batch_size=16, epochs=EPOCHS)
    return wav_corpus.write(n_train=N_TRAIN, n_test=N_TEST)


def read_history():
    with open("last_trained_model_results.json") as f:
        return json.load(f)


def test_cnn_train_against_colours_twice(wavs, capsys):
    argv = ["cnn", "train", "--engine", "hip", "--from-wav", "--augment-snrs", "20,0", "--augment-colours", "pink,speech", "--seed", "1"]
    assert cli.main(argv) == 0
    assert "speech 0dB" in capsys.readouterr().out
    h = read_history()
    weights = load_model("last_trained_model").ordered()
    n = len(h["loss"])
    assert set(h) == set(KEYS) | {"val_acc_snr", "val_loss_snr", "augment"} and n == EPOCHS
    assert len(h["val_acc_snr"]) == len(h["val_loss_snr"]) == 4 and all(len(per) == n for per in h["val_acc_snr"] + h["val_loss_snr"])
    a = h["augment"]
    assert a["colours"] == ["pink", "pink", "speech", "speech"] and a["level_snr_db"] == [20.0, 0.0, 20.0, 0.0]
    assert a["snrs"] == [20.0, 0.0] and a["noise_taps"] == 1025 and a["seed"] == 1 and len(set(a["noise_seed"])) == n
    print("history against colours", h)
    assert cli.main(argv) == 0
    assert read_history() == h
    for w0, w1 in zip(weights, load_model("last_trained_model").ordered()):
        assert np.asarray(w0).tobytes() == np.asarray(w1).tobytes()


def test_white_as_a_colour_trains_the_weights_of_the_snrs_alone(wavs):
    base = ["cnn", "train", "--engine", "hip", "--from-wav", "--augment-snrs", "20,0", "--seed", "1"]
    assert cli.main(base) == 0
    h0, w0 = read_history(), load_model("last_trained_model").ordered()
    assert cli.main(base + ["--augment-colours", "white"]) == 0
    h1, w1 = read_history(), load_model("last_trained_model").ordered()
    for a, b in zip(w0, w1):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    for k in h0:
        assert (h1[k] == h0[k]) if k != "augment" else all(h1[k][j] == h0[k][j] for j in h0[k]), k
    assert h1["augment"]["colours"] == ["white", "white"]


def test_every_epoch_sees_other_levels(wavs):
    """on_epoch: the rendered set before the steps of epochs 0 and 1; a file that drew the clean level has the clean render's
    windows. The levels are redrawn from default_rng([seed, NOISE_STREAM]) as TrainFromWav draws them, K = colours x SNRs."""
    seen = []
    Training.TrainFromWav(snrs=(20.0, 0.0), colours=("pink", "speech"), seed=1, verbose=0, on_epoch=lambda it, t: seen.append(t.windows()[0]))
    x0, x1 = seen
    assert x0.shape == x1.shape == (N_TRAIN * wav_corpus.SEGMENTS, 11, 128) and np.isfinite(x0).all()
    assert not np.array_equal(x0, x1)
    seen.clear()
    Training.TrainFromWav(seed=1, verbose=0, on_epoch=lambda it, t: seen.append(t.windows()[0]))
    clean = seen[0]
    rng = np.random.default_rng([1, Training.NOISE_STREAM])
    per = wav_corpus.SEGMENTS
    drawn = []
    for x in (x0, x1):
        level_of, _ = Training.draw_epoch_noise(rng, 4, N_TRAIN)
        drawn.append(level_of)
        for f, l in enumerate(level_of):
            assert np.array_equal(x[f * per:(f + 1) * per], clean[f * per:(f + 1) * per]) == (l == 4), (f, l)
    assert not np.array_equal(drawn[0], drawn[1])


def test_colours_and_rooms_together(wavs):
    argv = ["cnn", "train", "--engine", "hip", "--from-wav", "--augment-snrs", "10", "--augment-colours", "pink,brown", "--augment-noise-taps",
            "255", "--augment-t60", "0.05", "--seed", "2"]
    assert cli.main(argv) == 0
    h = read_history()
    assert set(h) == set(KEYS) | {"val_acc_snr", "val_loss_snr", "val_acc_room", "val_loss_room", "augment"}
    assert len(h["val_acc_snr"]) == 2 and len(h["val_acc_room"]) == 1
    a = h["augment"]
    assert a["colours"] == ["pink", "brown"] and a["noise_taps"] == 255 and a["t60"] == [0.05] and len(a["room_seed"]) == len(h["loss"])
