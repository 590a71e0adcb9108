"""Training at reduced resolution: Trainer.render(mixes=..., mix_of=...) against f2_input_batch_smeared group by group, against the
render without matrices, and `cnn train --engine hip --from-wav --augment-spreads ... --augment-bands ...` on a labelled WAV corpus
written into the test's own directory (tests/wav_corpus.py: 6 TRAIN and 2 TEST files of 1 s at the default configuration, windows
of 11 x 128), two epochs at batch 16. No accuracy is asserted, as in tests/test_gpu_train_colours.py: the assertions are about the
run, its files and its repeatability. (That the matrices go up once per render and not once per group is how
f2_trainer_render_smeared is written; nothing a caller can observe tells the two apart, so no test here does.)"""
import json

import numpy as np
import pytest

import f2cnn_oracle as orc
import noisy_batch as nb
import train_referee as tr
import wav_corpus
from f2cnn_amd import _lib, cli, config, smear
from f2cnn_amd.config import F2Config
from f2cnn_amd.model import F2CNNModel, load_model
from f2cnn_amd.reverb import SyntheticRIR
from f2cnn_amd.scripts.CNN import Training
from f2cnn_amd.trainer import Trainer
from noisy_batch import C, R, RADIUS, SEED, SNR, STEP, bits
from test_gpu_shaped_noise import random_filter

pytestmark = pytest.mark.gpu

NB = 5                                          # the first five utterances of tests/noisy_batch.py: groups of 2, 2 and 1
GROUP = 2
FIRS = [random_filter(t, 3) for t in (5, 1025, 2048)]
RIRS = [SyntheticRIR(1.0, t, seed=9, level=l) for l, t in enumerate((7, 1025))]
ROOM_OF = (1, 2, 0, 2, 0)
LEVEL_OF = nb.LEVEL_OF[:NB]
KM = 3
MIX_OF = (2, 0, 1, 3, 1)                        # every matrix and the sharp level
EPOCHS, N_TRAIN, N_TEST = 2, 6, 2
KEYS = ("loss", "acc", "val_loss", "val_acc")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    with c.options(spectral_min_rows=0):
        yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    flat, offsets = nb.waves()
    cs, _ = nb.centers()
    rng = np.random.default_rng(3)
    return [flat[offsets[b]:offsets[b + 1]] for b in range(NB)], cs[:NB], [rng.integers(0, 2, len(c)).astype(np.uint8) for c in cs[:NB]]


def matrices():
    freqs = orc.centre_freqs(16000, C, 100)
    return np.stack([smear.SmearMatrix(freqs, 1.0), smear.BandMatrix(C, 6), smear.SmearMatrix(freqs, 3.0)])


def new_trainer(ctx):
    return Trainer(F2CNNModel.glorot(7, R, C, zero_bias=False), lr=1e-3, rho=0.9, eps=1e-7, decay=0.5, drop=tr.DROP, seed=5, ctx=ctx)


@pytest.mark.parametrize("stages", ("alone", "all"))
def test_render_with_matrices_is_input_batch_smeared_group_by_group(ctx, corpus, stages):
    waves, cs, signs = corpus
    flat, offsets = nb.waves()
    coefs, mix = nb.coefs(), matrices()
    full = stages == "all"
    room, lev, mof = np.array(ROOM_OF, np.int32), np.array(LEVEL_OF, np.int32), np.array(MIX_OF, np.int32)
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, coefs, RADIUS, STEP, lpf=True, cutoff=50.0, group=GROUP)

    def render(mixes=mix, mix_of=mof):
        if full:
            t.render_wet(RIRS, room, SNR, lev, SEED, firs=FIRS, mixes=mixes, mix_of=mix_of)
        else:
            t.render(mixes=mixes, mix_of=mix_of)
    render()
    x, y = t.windows()
    assert np.array_equal(y, np.concatenate(signs)) and np.isfinite(x).all()
    row = 0
    for g in range(0, NB, GROUP):                             # group g starts at first_utterance = g; the last one is partial
        e = min(g + GROUP, NB)
        part = flat[int(offsets[g]):int(offsets[e])]
        coff = np.concatenate([[0], np.cumsum([len(c) for c in cs[g:e]])]).astype(np.int64)
        want = np.full((int(coff[-1]), R, C), np.nan, np.float32)
        if len(want):
            ctx.input_batch_smeared(part, _lib.WAVE_I16, offsets[g:e + 1] - offsets[g], coefs, e - g, C, True, 50.0, _lib.FFT_F32, coff,
                                    np.concatenate(cs[g:e]), RADIUS, STEP, True, RIRS if full else (), room[g:e] if full else None,
                                    SNR if full else (), FIRS if full else None, lev[g:e] if full else None, g, SEED if full else 0, mix,
                                    mof[g:e], want, _lib.MEM_HOST)
        assert bits(x[row:row + len(want)]).tobytes() == bits(want).tobytes(), g
        row += len(want)
    assert row == len(x)
    # a second render: the same bytes; a bad level or weight: an error that names it and changes nothing
    render()
    assert bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    bad = mof.copy()
    bad[3] = KM + 1
    with pytest.raises(_lib.F2Error, match="utterance 3") as ei:
        render(mix_of=bad)
    assert ei.value.code == _lib.F2_ERR_INVALID and bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    nan = mix.copy()
    nan[1, 2, 3] = np.nan
    with pytest.raises(_lib.F2Error) as ei:
        render(mixes=nan)
    assert ei.value.code == _lib.F2_ERR_INVALID and "[1][2][3]" in str(ei.value) and bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    t.close()


def test_the_groups_of_a_render_share_nothing_they_change(ctx):
    """Rooms, coloured noise and matrices at once on a trainer in groups of two over five utterances (radius 5, step 160, windows of
    11 x 10: the narrowest network with a dense1 input; 1761, 2500, 1000 - no room for a window -, 2100 and 1900 samples): the middle
    group entirely dry, clean and sharp between two that are not, the last one partial. Rendered twice with the same arguments the
    bytes are the same, and each group is f2_input_batch_smeared on its utterances with first_utterance = the group's first."""
    Cs, rad, stp, lens = 10, 5, 160, (1761, 2500, 1000, 2100, 1900)
    reach, rows = rad * stp, 2 * rad + 1
    waves = [orc.synth_utterance(70 + i, n).astype(np.int16) for i, n in enumerate(lens)]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cs = [np.array([reach, n // 2, n - 1 - reach], np.int64) if n > 2 * reach else np.zeros(0, np.int64) for n in lens]
    signs = [(np.arange(len(c)) % 2).astype(np.uint8) for c in cs]
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, Cs, 100))
    freqs = orc.centre_freqs(16000, Cs, 100)
    mix = np.stack([smear.SmearMatrix(freqs, 1.0), smear.BandMatrix(Cs, 3), smear.SmearMatrix(freqs, 3.0)])
    K, KR = len(SNR), len(RIRS)
    room, lev, mof = np.array((1, 0, KR, KR, 1), np.int32), np.array((0, 2, K, K, 1), np.int32), np.array((2, 0, KM, KM, 1), np.int32)
    t = Trainer(F2CNNModel.glorot(7, rows, Cs, zero_bias=False), lr=1e-3, rho=0.9, eps=1e-7, decay=0.5, drop=tr.DROP, seed=5, ctx=ctx)
    t.set_waves(waves, cs, signs, coefs, rad, stp, lpf=True, cutoff=50.0, group=GROUP)
    t.render_wet(RIRS, room, SNR, lev, SEED, firs=FIRS, mixes=mix, mix_of=mof)
    x, y = t.windows()
    assert np.array_equal(y, np.concatenate(signs)) and len(x) == 12 and np.isfinite(x).all()
    t.render_wet(RIRS, room, SNR, lev, SEED, firs=FIRS, mixes=mix, mix_of=mof)
    assert bits(t.windows()[0]).tobytes() == bits(x).tobytes()
    flat, row = np.concatenate(waves), 0
    for g in range(0, len(lens), GROUP):
        e = min(g + GROUP, len(lens))
        coff = np.concatenate([[0], np.cumsum([len(c) for c in cs[g:e]])]).astype(np.int64)
        want = np.full((int(coff[-1]), rows, Cs), np.nan, np.float32)
        ctx.input_batch_smeared(flat[int(offsets[g]):int(offsets[e])], _lib.WAVE_I16, offsets[g:e + 1] - offsets[g], coefs, e - g, Cs, True, 50.0,
                                _lib.FFT_F32, coff, np.concatenate(cs[g:e]), rad, stp, True, RIRS, room[g:e], SNR, FIRS, lev[g:e], g, SEED, mix,
                                mof[g:e], want, _lib.MEM_HOST)
        assert len(want) == 3 * sum(n > 2 * reach for n in lens[g:e])
        assert bits(x[row:row + len(want)]).tobytes() == bits(want).tobytes(), g
        row += len(want)
    assert row == len(x)
    # the middle group is the plain render's: its windows carry no room, no noise and no mixing
    t.render()
    assert bits(t.windows()[0][6:9]).tobytes() == bits(x[6:9]).tobytes() and not np.array_equal(t.windows()[0][:6], x[:6])
    t.close()


def test_without_matrices_it_is_the_render_it_was(ctx, corpus):
    waves, cs, signs = corpus
    mix = matrices()
    t = new_trainer(ctx)
    t.set_waves(waves, cs, signs, nb.coefs(), RADIUS, STEP, group=GROUP)
    t.render_wet(RIRS, ROOM_OF, SNR, LEVEL_OF, SEED, firs=FIRS)
    old, _ = t.windows()
    t.render()
    clean, _ = t.windows()
    assert not np.array_equal(old, clean)
    t.render_wet(RIRS, ROOM_OF, SNR, LEVEL_OF, SEED, firs=FIRS, mixes=None)
    assert bits(t.windows()[0]).tobytes() == bits(old).tobytes()
    for mixes, mix_of in ((None, None), (mix, None), (None, MIX_OF), (mix, (KM,) * NB)):
        ctx.trainer_render_smeared(t.handle, RIRS, ROOM_OF, SNR, FIRS, LEVEL_OF, SEED, mixes, mix_of, C)
        assert bits(t.windows()[0]).tobytes() == bits(old).tobytes(), mix_of
    t.render(mixes=mix, mix_of=(KM,) * NB)
    assert bits(t.windows()[0]).tobytes() == bits(clean).tobytes()
    # ... and matrices are not
    t.render(mixes=mix, mix_of=MIX_OF)
    assert not np.array_equal(t.windows()[0], clean)
    t.close()


@pytest.fixture()
def wavs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    config.write_default(batch_size=16, epochs=EPOCHS)
    return wav_corpus.write(n_train=N_TRAIN, n_test=N_TEST)


def read_history():
    with open("last_trained_model_results.json") as f:
        return json.load(f)


def test_cnn_train_at_reduced_resolution_twice(wavs, capsys):
    argv = ["cnn", "train", "--engine", "hip", "--from-wav", "--augment-spreads", "1,4", "--augment-bands", "8", "--seed", "1"]
    assert cli.main(argv) == 0
    assert "1ERB" in capsys.readouterr().out
    h = read_history()
    weights = load_model("last_trained_model").ordered()
    n = len(h["loss"])
    assert set(h) == set(KEYS) | {"val_acc_smear", "val_loss_smear", "augment"} and n == EPOCHS
    assert len(h["val_acc_smear"]) == len(h["val_loss_smear"]) == 3 and all(len(per) == n for per in h["val_acc_smear"] + h["val_loss_smear"])
    a = h["augment"]
    assert a["spreads"] == [1.0, 4.0] and a["bands"] == [8] and a["smear_levels"] == ["1ERB", "4ERB", "8bands"] and a["seed"] == 1
    print("history at reduced resolution", h)
    assert cli.main(argv) == 0
    assert read_history() == h
    for w0, w1 in zip(weights, load_model("last_trained_model").ordered()):
        assert np.asarray(w0).tobytes() == np.asarray(w1).tobytes()


def test_every_epoch_sees_the_drawn_resolutions(wavs):
    """on_epoch: the rendered set before the steps of epochs 0 and 1 is one f2_input_batch_smeared of the TRAIN files at the levels
    redrawn here from default_rng([seed, SMEAR_STREAM]), with TrainFromWav's own matrices"""
    from f2cnn_amd.scripts.processing.EnvelopeExtraction import FFT_PRECISION
    from f2cnn_amd.scripts.processing.GammatoneFiltering import filterbank_from_config
    seen = []
    Training.TrainFromWav(spreads=(1.0, 4.0), bands=(8,), seed=1, verbose=0, on_epoch=lambda it, t: seen.append(t.windows()[0]))
    assert len(seen) == EPOCHS and not np.array_equal(seen[0], seen[1])
    cfg = F2Config()
    freqs, coefs = filterbank_from_config(cfg)
    coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    mixes, names = Training.build_smear_levels((1.0, 4.0), (8,), freqs)
    assert names == ["1ERB", "4ERB", "8bands"]
    lw = Training.LabelledWaves("trainingData/label_data.csv")
    waves = lw.read(cfg.radius * cfg.step)
    train = lw.split(False)
    flat = np.concatenate([waves[k] for k in train])
    offsets = np.concatenate([[0], np.cumsum([len(waves[k]) for k in train])]).astype(np.int64)
    coff = np.concatenate([[0], np.cumsum([len(lw.centers[k]) for k in train])]).astype(np.int64)
    rng = np.random.default_rng([1, Training.SMEAR_STREAM])
    ctx = _lib.default_context()
    drawn = []
    for x in seen:
        mix_of = Training.draw_epoch_smear(rng, 3, len(train))
        drawn.append(mix_of)
        want = np.full(x.shape, np.nan, np.float32)
        ctx.input_batch_smeared(flat, _lib.WAVE_I16, offsets, coefs, len(train), coefs.shape[0], False, 0.0, FFT_PRECISION, coff,
                                np.concatenate([lw.centers[k] for k in train]), cfg.radius, cfg.step, True, (), None, (), None, None, 0, 0,
                                mixes, mix_of, want, _lib.MEM_HOST)
        assert bits(x).tobytes() == bits(want).tobytes()
    assert not np.array_equal(drawn[0], drawn[1])


def test_without_the_new_arguments_the_run_is_the_one_it_was(wavs):
    """TrainFromWav(snrs=...) against the epoch loop written out with the calls that were there before the spectral resolutions:
    the noise generator is drawn as before and the weights are the same bytes"""
    from f2cnn_amd.scripts.processing.EnvelopeExtraction import FFT_PRECISION
    from f2cnn_amd.scripts.processing.GammatoneFiltering import filterbank_from_config
    snrs = (20.0, 0.0)
    model, history = Training.TrainFromWav(snrs=snrs, seed=1, verbose=0)
    assert "val_acc_smear" not in history and len(history["loss"]) == EPOCHS
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
        trainer.render(snrs, level_of, noise_seed)
        trainer.steps(rng.permutation(n), 16)
    old = trainer.model()
    for w0, w1 in zip(old.ordered(), model.ordered()):
        assert np.asarray(w0).tobytes() == np.asarray(w1).tobytes()
    trainer.close()
