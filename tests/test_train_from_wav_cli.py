"""`cnn train --engine hip --from-wav [--augment-snrs ...]`: the parts that need no GPU - the two flags on the command line and
what it refuses, the keywords main() hands to TrainFromWav, the five entry points in the header and the ctypes table, LabelledWaves on
a written corpus, and the per-epoch draw of the noise conditions."""
import ctypes
import os
import re

import numpy as np
import pytest

import wav_corpus
from conftest import ROOT
from f2cnn_amd import _lib, cli
from f2cnn_amd.scripts.CNN import Training


def test_the_flags_parse_and_are_absent_unless_given():
    plain = vars(cli.build_parser().parse_args(["cnn", "train"]))
    assert "from_wav" not in plain and "augment_snrs" not in plain and "engine" not in plain
    args = cli.build_parser().parse_args(["cnn", "train", "--engine", "hip", "--from-wav", "--augment-snrs", "20,10,5,0", "--seed", "4",
                                          "--lpf", "50"])
    assert args.from_wav is True and args.augment_snrs == [20.0, 10.0, 5.0, 0.0] and args.seed == 4 and args.CUTOFF == 50
    only = vars(cli.build_parser().parse_args(["cnn", "train", "--engine", "hip", "--from-wav"]))
    assert only["from_wav"] is True and "augment_snrs" not in only
    assert "--from-wav" in cli.__doc__ and "--augment-snrs" in cli.__doc__


@pytest.mark.parametrize("bad", ["20,x", "", "nan", "3,,1"])
def test_a_malformed_list_is_refused_by_the_parser(bad, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["cnn", "train", "--engine", "hip", "--from-wav", "--augment-snrs", bad])
    assert e.value.code == 2 and "--augment-snrs" in capsys.readouterr().err


REFUSALS = [(["cnn", "train", "--engine", "hip", "--augment-snrs", "20,3"], "--augment-snrs needs --from-wav"),
            (["cnn", "train", "--from-wav"], "--from-wav needs --engine hip"),
            (["cnn", "train", "--engine", "torch", "--from-wav"], "--from-wav needs --engine hip"),
            (["cnn", "train", "--augment-snrs", "20"], "--augment-snrs needs --engine hip"),
            (["cnn", "train", "--engine", "torch", "--from-wav", "--augment-snrs", "20"], "--from-wav needs --engine hip"),
            (["cnn", "eval", "--file", "a.WAV", "--from-wav"], "--from-wav only applies to 'cnn train'"),
            (["cnn", "test", "--augment-snrs", "20"], "--augment-snrs only applies to 'cnn train'"),
            (["cnn", "noisesweep", "--file", "a.WAV", "--snrs", "3", "--engine", "hip", "--from-wav"], "--from-wav only applies to 'cnn train'")]


@pytest.mark.parametrize("argv,message", REFUSALS)
def test_refusals_touch_nothing(argv, message, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    called = []
    monkeypatch.setattr(Training, "TrainFromWav", lambda **kw: called.append(kw))
    monkeypatch.setattr(Training, "TrainAndPlotLoss", lambda **kw: called.append(kw))
    monkeypatch.setattr(_lib, "default_context", lambda *a, **k: pytest.fail("a refused command line opened the device"))
    assert cli.main(argv) != 0
    assert message in capsys.readouterr().out
    assert not called and os.listdir(tmp_path) == []


def test_main_hands_the_options_to_TrainFromWav(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    called = []
    monkeypatch.setattr(Training, "TrainFromWav", lambda **kw: called.append(kw))
    assert cli.main(["cnn", "train", "--engine", "hip", "--from-wav"]) == 1          # no label file yet
    assert "prepare label" in capsys.readouterr().out and not called
    os.makedirs("trainingData")
    open(os.path.join("trainingData", "label_data.csv"), "w").close()
    assert cli.main(["cnn", "train", "--engine", "hip", "--from-wav"]) == 0
    assert called.pop() == dict(labelFile=os.path.join("trainingData", "label_data.csv"), LPF=False, CUTOFF=None, snrs=(), seed=None)
    open("mine.csv", "w").close()
    assert cli.main(["cnn", "train", "--engine", "hip", "--from-wav", "--augment-snrs", "20,3", "--seed", "9", "--lpf", "50", "-l", "mine.csv"]) == 0
    assert called.pop() == dict(labelFile="mine.csv", LPF=True, CUTOFF=50, snrs=(20.0, 3.0), seed=9)


def test_cnn_train_without_the_flags_is_todays_call(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    called = []
    monkeypatch.setattr(Training, "TrainAndPlotLoss", lambda **kw: called.append(kw))
    monkeypatch.setattr(Training, "TrainFromWav", lambda **kw: pytest.fail("not asked for"))
    os.makedirs("trainingData")
    for name in ("label_data.csv", "last_input_data.npy"):
        open(os.path.join("trainingData", name), "w").close()
    assert cli.main(["cnn", "train", "--engine", "hip"]) == 0
    assert called == [dict(labelFile=os.path.join("trainingData", "label_data.csv"),
                           inputFile=os.path.join("trainingData", "last_input_data.npy"), engine="hip")]


def test_the_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {"f2_noise_pick": 13, "f2_input_batch_noisy": 22, "f2_trainer_set_waves": 17, "f2_trainer_render": 6, "f2_trainer_get_windows": 6}
    for name, n in counts.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(params) == len(args) == n, name
        for p, a in zip(params, args):
            if p.startswith("uint64_t "):
                assert a is ctypes.c_uint64, (name, p)
            elif p.startswith("uint32_t "):
                assert a is ctypes.c_uint32, (name, p)
            elif p.startswith("int64_t "):
                assert a is ctypes.c_int64, (name, p)
            elif p.startswith("int "):
                assert a is ctypes.c_int, (name, p)
            elif p.startswith("double "):
                assert a is ctypes.c_double, (name, p)
            else:
                assert "*" in p and a is ctypes.c_void_p, (name, p)
        assert hasattr(_lib.Context, name[len("f2_"):])
    # f2_input_batch_noisy is f2_input_batch's list with the five noise arguments before the output
    assert _lib.SIGNATURES["f2_input_batch_noisy"][1][:16] == _lib.SIGNATURES["f2_input_batch"][1][:16]
    for word in ("Evaluating.py:193-221", "Training.py:129-134"):
        assert word in text, word


def test_labelled_waves(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    files = wav_corpus.write(n_train=3, n_test=2)
    lw = Training.LabelledWaves(os.path.join("trainingData", "label_data.csv"))
    assert lw.keys == sorted(k.replace("/", os.sep) + ".ENV1.npy" for k in files) and len(lw) == 5
    assert lw.is_test == [True, True, False, False, False] and lw.split(True) == [0, 1] and lw.split(False) == [2, 3, 4]
    for key, wav, centres, signs in zip(lw.keys, lw.wavs, lw.centers, lw.signs):
        wave, want_centres, want_signs = files[key[:-len(".ENV1.npy")].replace(os.sep, "/")]
        assert wav == os.path.join("resources", "f2cnn", key[:-len(".ENV1.npy")] + ".WAV") and os.path.isfile(wav)
        assert centres.dtype == np.int64 and np.array_equal(centres, want_centres)          # CSV order inside the file
        assert signs.dtype == np.uint8 and np.array_equal(signs, want_signs)
    waves = lw.read(800)
    for key, w in zip(lw.keys, waves):
        assert w.dtype == np.int16 and np.array_equal(w, files[key[:-len(".ENV1.npy")].replace(os.sep, "/")][0])
    # a window outside its file, with `prepare input --from-wav`'s message
    with open(os.path.join("trainingData", "label_data.csv"), "a") as f:
        f.write("TEST,DR1,F0000,SX2,aa,15500,0.5,0.01,1\n")
    with pytest.raises(ValueError, match=r"DR1\.F0000\.SX2\.WAV: the window at timepoint 15500 \(\+-800 samples\) reaches outside its 16000"):
        Training.LabelledWaves(os.path.join("trainingData", "label_data.csv")).read(800)
    # a label key without its WAV
    with open(os.path.join("trainingData", "label_data.csv"), "a") as f:
        f.write("TRAIN,DR9,MZZZ0,SA1,aa,5000,0.5,0.01,0\n")
    with pytest.raises(FileNotFoundError, match=r"DR9\.MZZZ0\.SA1\.WAV \(label key .*\) does not exist"):
        Training.LabelledWaves(os.path.join("trainingData", "label_data.csv"))
    with open("bad.csv", "w") as f:
        f.write("TRAIN,DR1,M0000,SA1,aa,5000,0.5,0.01,2\n")
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        Training.LabelledWaves("bad.csv")


def test_the_epoch_draw_is_reproducible_and_covers_every_level():
    K, B = 3, 40
    def run(seed, epochs=6):
        rng = np.random.default_rng([seed, Training.NOISE_STREAM])
        return [Training.draw_epoch_noise(rng, K, B) for _ in range(epochs)]
    a, b, c = run(3), run(3), run(4)
    assert Training.NOISE_STREAM == 0x6E6F6973
    for (la, sa), (lb, sb) in zip(a, b):
        assert la.dtype == np.int32 and la.shape == (B,) and np.array_equal(la, lb) and sa == sb and 0 <= sa < 2 ** 63
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(a, c)) and [s for _, s in a] != [s for _, s in c]
    assert len({s for _, s in a}) == len(a)
    levels = np.concatenate([l for l, _ in a])
    assert set(levels.tolist()) == set(range(K + 1))                  # every level and the clean one, nothing else
    # the order of the two draws is part of the format: levels first, then the seed
    rng = np.random.default_rng([3, Training.NOISE_STREAM])
    assert np.array_equal(rng.integers(0, K + 1, B), a[0][0]) and int(rng.integers(0, 2 ** 63)) == a[0][1]
