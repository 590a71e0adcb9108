"""Training windows straight from the waves (f2_input_batch, `prepare input --from-wav`): bit-identical to the fused
filterbank + envelope call followed by K3 per utterance, one gather launch per call, the edges of the ragged batch, and
the file command against `prepare features` + `prepare input`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import f2cnn_oracle as orc
from conftest import chan_relerr
from f2cnn_amd import _lib, cli, config, wavio

pytestmark = pytest.mark.gpu

C, RADIUS, STEP = 128, 5, 160
REACH = RADIUS * STEP
R = 2 * RADIUS + 1
# one length per envelope route: short (filterbank + envelope kernels), KS, exactly 2^k (two-kernel), KSL, four-step
LENGTHS = (3000, 16000, 16384, 40000, 70000)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coefs():
    return orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))


def make_batch(lengths, seed=7):
    waves = [orc.synth_utterance(seed + i, n) for i, n in enumerate(lengths)]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return waves, offs


def make_centers(lengths, per=(3, 5, 2, 7, 4), seed=11):
    """per[b] centres inside utterance b's legal range [REACH, n_b - 1 - REACH], both ends included where there is room"""
    rng = np.random.default_rng(seed)
    cs = []
    for b, n in enumerate(lengths):
        k = per[b % len(per)]
        if k == 0 or n < 2 * REACH + 1:
            cs.append(np.zeros(0, np.int64))
            continue
        c = rng.integers(REACH, n - REACH, size=k)
        c[0] = REACH
        if k > 1:
            c[-1] = n - 1 - REACH
        cs.append(c.astype(np.int64))
    coffs = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    return cs, coffs


def input_batch(ctx, flat, dt, offs, coefs, lpf, cutoff, precision, cs, coffs, normalize, mem=_lib.MEM_HOST):
    nwin = int(coffs[-1])
    out = np.full((nwin, R, C), np.nan, np.float32)
    centers = np.concatenate(cs).astype(np.int64) if cs else np.zeros(0, np.int64)
    if mem == _lib.MEM_HOST:
        ctx.input_batch(flat, dt, offs, coefs, len(offs) - 1, C, lpf, cutoff, precision, coffs, centers, RADIUS, STEP,
                        normalize, out, _lib.MEM_HOST)
        return out
    import torch
    d_wave = torch.from_numpy(flat).cuda()
    d_out = torch.full((max(nwin, 1), R, C), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.input_batch(d_wave.data_ptr(), dt, offs, coefs, len(offs) - 1, C, lpf, cutoff, precision, coffs, centers, RADIUS,
                    STEP, normalize, d_out.data_ptr(), _lib.MEM_DEVICE)
    ctx.synchronize()
    return d_out[:nwin].cpu().numpy()


def two_step(ctx, flat, dt, offs, coefs, lpf, cutoff, precision, cs, normalize):
    """f2_filterbank_envelope_fused (gfb = NULL) on the same batch, then f2_gather_windows per utterance"""
    env = np.empty(C * int(offs[-1]))
    ctx.filterbank_envelope_fused(flat, dt, offs, coefs, len(offs) - 1, C, lpf, cutoff, precision, env, None, _lib.MEM_HOST)
    out = []
    for b, c in enumerate(cs):
        if len(c):
            e = env[C * offs[b]:C * offs[b + 1]].reshape(C, -1)
            w = np.empty((len(c), R, C), np.float32)
            ctx.gather_windows(e, C, e.shape[1], np.ascontiguousarray(c), len(c), RADIUS, STEP, normalize, w, _lib.MEM_HOST)
            out.append(w)
    return np.concatenate(out) if out else np.zeros((0, R, C), np.float32), env


CASES = [(lpf, norm, dt, _lib.FFT_F32, _lib.MEM_HOST) for lpf in (0, 50) for norm in (0, 1)
         for dt in (_lib.WAVE_I16, _lib.WAVE_F64)]
CASES += [(50, 0, _lib.WAVE_I16, _lib.FFT_F64, _lib.MEM_HOST), (50, 0, _lib.WAVE_I16, _lib.FFT_F32, _lib.MEM_DEVICE),
          (0, 1, _lib.WAVE_F64, _lib.FFT_F32, _lib.MEM_DEVICE)]


@pytest.mark.parametrize("lpf,normalize,dt,precision,mem", CASES)
def test_input_batch_bit_identical_to_fused_then_gather(ctx, coefs, lpf, normalize, dt, precision, mem):
    waves, offs = make_batch(LENGTHS)
    flat = np.concatenate(waves)
    if dt == _lib.WAVE_F64:
        flat = flat.astype(np.float64) * 0.37
    cs, coffs = make_centers(LENGTHS)
    with ctx.options(spectral_min_rows=0):
        got = input_batch(ctx, flat, dt, offs, coefs, bool(lpf), float(lpf), precision, cs, coffs, normalize, mem)
        routed = ctx.get_option("spectral_routed")
        want, _ = two_step(ctx, flat, dt, offs, coefs, bool(lpf), float(lpf), precision, cs, normalize)
    if precision == _lib.FFT_F32:
        assert routed == 2, routed             # 16000 and 40000 samples took the spectral kernel (KS / KSL)
    assert got.shape == (int(coffs[-1]), R, C)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("normalize", [0, 1])
def test_input_batch_matches_oracle(ctx, coefs, normalize):
    lengths = (3000, 16000, 40000)
    waves, offs = make_batch(lengths, seed=40)
    cs, coffs = make_centers(lengths, per=(2, 4, 3))
    with ctx.options(spectral_min_rows=0):
        got = input_batch(ctx, np.concatenate(waves), _lib.WAVE_I16, offs, coefs, True, 50.0, _lib.FFT_F32, cs, coffs,
                          normalize)
        _, env = two_step(ctx, np.concatenate(waves), _lib.WAVE_I16, offs, coefs, True, 50.0, _lib.FFT_F32, cs, 0)
    for b, w in enumerate(waves):
        ref = orc.gather_windows(orc.filter_and_envelope(w, coefs, True, 50), cs[b], RADIUS, STEP)
        mine = got[coffs[b]:coffs[b + 1]]
        if not normalize:
            for e in range(len(cs[b])):
                # per window, channels as rows (chan_relerr's norm)
                assert chan_relerr(mine[e].T, ref[e].T) <= 1e-5, (b, e)
            continue
        # normalizeInput of the oracle on the device's own envelopes: the float32 rounding of the same float64 arithmetic
        dev = orc.gather_windows(env[C * offs[b]:C * offs[b + 1]].reshape(C, -1), cs[b], RADIUS, STEP)
        np.testing.assert_allclose(mine, np.stack([orc.normalize_input(r) for r in dev]), rtol=0, atol=2e-7)
        # ... and on the oracle's envelopes: (ln v - ln min) / (ln max - ln min) turns the float32 FFT's error, 1e-7 of a
        # channel's maximum, into |dv| / v of the quietest samples - up to 8e-4 of the [0, 1] range measured here
        np.testing.assert_allclose(mine, np.stack([orc.normalize_input(r) for r in ref]), rtol=0, atol=2e-3)


def test_one_gather_launch_per_call(ctx, coefs):
    lengths = [16000 + 37 * i for i in range(16)]
    waves, offs = make_batch(lengths, seed=90)
    cs, coffs = make_centers(lengths)
    ctx.prof_enable(True)
    try:
        input_batch(ctx, np.concatenate(waves), _lib.WAVE_I16, offs, coefs, True, 50.0, _lib.FFT_F32, cs, coffs, 0)
        ran = ctx.prof_get()
    finally:
        ctx.prof_enable(False)
    assert ran["k_gather_windows"][0] == 1, ran


@pytest.mark.parametrize("per", [(0, 3, 2, 4, 5), (3, 0, 2, 4, 5), (3, 2, 0, 4, 5), (3, 2, 4, 5, 0), (0, 0, 0, 0, 0)])
def test_utterances_without_centres(ctx, coefs, per):
    lengths = (900, 16000, 2000, 40000, 500)       # the short ones are shorter than a window
    lengths = tuple(max(n, 2 * REACH + 1) if k else n for n, k in zip(lengths, per))
    waves, offs = make_batch(lengths, seed=3)
    flat = np.concatenate(waves)
    cs, coffs = make_centers(lengths, per=per)
    got = input_batch(ctx, flat, _lib.WAVE_I16, offs, coefs, True, 50.0, _lib.FFT_F32, cs, coffs, 0)
    want, _ = two_step(ctx, flat, _lib.WAVE_I16, offs, coefs, True, 50.0, _lib.FFT_F32, cs, 0)
    assert got.shape == want.shape == (sum(per), R, C)
    np.testing.assert_array_equal(got, want)


def test_empty_batch(ctx, coefs):
    out = np.full((1, R, C), 7.0, np.float32)
    ctx.input_batch(np.zeros(1, np.int16), _lib.WAVE_I16, np.zeros(1, np.int64), coefs, 0, C, True, 50.0, _lib.FFT_F32,
                    np.zeros(1, np.int64), np.zeros(0, np.int64), RADIUS, STEP, 0, out, _lib.MEM_HOST)
    assert (out == 7.0).all()


def test_window_edges(ctx, coefs):
    lengths = (16000, 20000)
    waves, offs = make_batch(lengths, seed=5)
    flat = np.concatenate(waves)

    def run(c1):
        cs = [np.array([REACH, 8000], np.int64), np.array(c1, np.int64)]
        return input_batch(ctx, flat, _lib.WAVE_I16, offs, coefs, False, 0.0, _lib.FFT_F32, cs,
                           np.array([0, 2, 2 + len(c1)], np.int64), 0), cs
    got, cs = run([REACH, lengths[1] - 1 - REACH])            # the first and the last legal centre
    want, _ = two_step(ctx, flat, _lib.WAVE_I16, offs, coefs, False, 0.0, _lib.FFT_F32, cs, 0)
    np.testing.assert_array_equal(got, want)
    for bad in (REACH - 1, lengths[1] - REACH):
        with pytest.raises(_lib.F2Error) as ei:
            run([9000, bad])
        assert ei.value.code == _lib.F2_ERR_INVALID
        msg = str(ei.value)
        assert "utterance 1" in msg and str(bad) in msg and str(lengths[1]) in msg, msg


def test_zero_window_normalized_is_nonpositive(ctx, coefs):
    n = 16000
    wave = np.zeros(n, np.int16)                    # silence: an all-zero envelope
    out = np.empty((1, R, C), np.float32)
    with pytest.raises(_lib.F2Error) as ei:
        ctx.input_batch(wave, _lib.WAVE_I16, np.array([0, n], np.int64), coefs, 1, C, False, 0.0, _lib.FFT_F32,
                        np.array([0, 1], np.int64), np.array([5000], np.int64), RADIUS, STEP, 1, out, _lib.MEM_HOST)
    assert ei.value.code == _lib.F2_ERR_NONPOSITIVE


# ---- the file command ----
def write_corpus(lens):
    from scipy.io import wavfile
    config.write_default()
    for i, (key, n) in enumerate(sorted(lens.items())):
        os.makedirs(os.path.join("resources", "f2cnn", os.path.dirname(key)), exist_ok=True)
        w = orc.synth_utterance(500 + i, n)
        path = os.path.join("resources", "f2cnn", key + ".WAV")
        if i % 3 == 1:
            wavfile.write(path, 16000, w)            # RIFF
        else:
            wavio.write_sphere(path, 16000, w)       # NIST SPHERE, like TIMIT


def write_labels(lens, seed=1, path="trainingData/label_data.csv"):
    """every file labelled, rows of the files interleaved (CSV order is not file order)"""
    rng = np.random.default_rng(seed)
    rows = []
    for key, n in lens.items():
        tt, rest = key.split("/")
        region, speaker, sentence = rest.split(".")
        for tp in rng.integers(REACH, n - REACH, size=int(rng.integers(1, 6))):
            rows.append((tt, region, speaker, sentence, "aa", int(tp)))
    rng.shuffle(rows)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for r in rows:
            f.write(",".join(map(str, r)) + ",0.5,0.01,1\n")


CORPUS = {"TEST/DR1.FAAA0.SA1": 16000, "TEST/DR1.FBBB0.SX2": 25000, "TEST/DR3.MDDD0.SI9": 80000,
          "TRAIN/DR2.MCCC0.SI3": 48000, "TRAIN/DR2.MCCC0.SX4": 16384, "TRAIN/DR4.FEEE0.SA2": 33000,
          "TRAIN/DR5.MFFF0.SX7": 72000, "TRAIN/DR1.FGGG0.SI1": 20000}


def test_prepare_input_from_wav_cli(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    write_corpus(CORPUS)
    write_labels(CORPUS)
    assert cli.main(["prepare", "input", "--from-wav", "--cutoff", "50", "--metrics", "m.json"]) == 0
    x = np.load("trainingData/input_data_LPF50.npy")
    np.testing.assert_array_equal(x, np.load("trainingData/last_input_data.npy"))
    import glob
    import json
    assert not glob.glob("resources/f2cnn/*/*.GFB.npy") and not glob.glob("resources/f2cnn/*/*.ENV1.npy")
    m = json.load(open("m.json"))
    assert m["files"] == len(CORPUS) and abs(m["audio_seconds"] - sum(CORPUS.values()) / 16000) < 1e-3
    # the two-step path on the same corpus: `prepare features` writes the envelopes, `prepare input` gathers them. Both
    # commands take the whole 8-file corpus as ONE batch (their default batch sizes are 16 and 64 files), so the
    # envelopes come from the same routes (1024 rows: below spectral_min_rows, the filterbank + envelope kernels) and
    # the rows are asserted bit-identical
    from f2cnn_amd.scripts.processing.EnvelopeExtraction import FilterAndExtractAll
    FilterAndExtractAll(LPF=True, CUTOFF=50, keep_gfb=False)
    assert cli.main(["prepare", "input", "--cutoff", "50", "--input", "trainingData/two_step.npy"]) == 0
    np.testing.assert_array_equal(x, np.load("trainingData/two_step.npy"))
    assert x.shape[1:] == (R, C) and x.dtype == np.float32 and len(x) > len(CORPUS)
    # no --cutoff: no low-pass, the NOLPF file
    for f in glob.glob("resources/f2cnn/*/*.ENV1.npy"):
        os.remove(f)
    assert cli.main(["prepare", "input", "--from-wav"]) == 0
    y = np.load("trainingData/input_data_NOLPF.npy")
    assert y.shape == x.shape and not np.array_equal(x, y)
    assert not glob.glob("resources/f2cnn/*/*.ENV1.npy")


def test_prepare_input_from_wav_batches_of_other_sizes(tmp_path, monkeypatch):
    """Batches that differ from the two-step path's (and a batch large enough for the spectral kernel): within 1e-6 of the
    envelope maximum per window"""
    monkeypatch.chdir(tmp_path)
    lens = {"TRAIN/DR{}.M{:03d}0.SA1".format(1 + i % 4, i): 6000 + 271 * i for i in range(36)}
    write_corpus(lens)
    write_labels(lens, seed=2)
    from f2cnn_amd.scripts.processing.EnvelopeExtraction import FilterAndExtractAll
    from f2cnn_amd.scripts.processing.InputGenerator import GenerateInputDataFromWav
    FilterAndExtractAll(LPF=True, CUTOFF=50, keep_gfb=False)
    assert cli.main(["prepare", "input", "--cutoff", "50", "--input", "trainingData/two_step.npy"]) == 0
    want = np.load("trainingData/two_step.npy")
    for batch in (36, 7):        # 36 files x 128 rows: the spectral kernel; 7: the two-kernel route in other batches
        GenerateInputDataFromWav(LPF=True, CUTOFF=50, batch_files=batch)
        got = np.load("trainingData/input_data_LPF50.npy")
        assert got.shape == want.shape
        err = (np.abs(got.astype(np.float64) - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))).max()
        assert err <= 1e-6, (batch, err)


def test_prepare_input_from_wav_errors(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    write_corpus(CORPUS)
    write_labels(dict(CORPUS, **{"TRAIN/DR9.MZZZ0.SA1": 16000}))
    with pytest.raises(FileNotFoundError, match="DR9.MZZZ0.SA1.WAV"):
        cli.main(["prepare", "input", "--from-wav", "--cutoff", "50"])
    write_labels(CORPUS)
    with open("trainingData/label_data.csv", "a") as f:
        f.write("TEST,DR1,FAAA0,SA1,aa,15500,0.5,0.01,1\n")     # 15500 + 800 >= 16000 samples
    with pytest.raises(ValueError, match=r"DR1\.FAAA0\.SA1\.WAV.*15500"):
        cli.main(["prepare", "input", "--from-wav", "--cutoff", "50"])
    assert not os.path.exists("trainingData/input_data_LPF50.npy")


def test_two_ranks_one_device(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    write_corpus(CORPUS)
    write_labels(CORPUS)
    assert cli.main(["prepare", "input", "--from-wav", "--cutoff", "50"]) == 0
    single = open("trainingData/input_data_LPF50.npy", "rb").read()
    os.remove("trainingData/input_data_LPF50.npy")
    os.remove("trainingData/last_input_data.npy")
    procs = [subprocess.Popen([sys.executable, "-m", "f2cnn_amd", "prepare", "input", "--from-wav", "--cutoff", "50"],
                              env=dict(os.environ, F2CNN_RANK=str(r), F2CNN_WORLD="2", F2CNN_DEVICE="0",
                                       F2CNN_RUN_ID="from_wav_test", PYTHONPATH=os.pathsep.join(sys.path)),
                              stdout=subprocess.DEVNULL, stderr=subprocess.PIPE) for r in (1, 0)]
    for pr in procs:
        _, err = pr.communicate(timeout=600)
        assert pr.returncode == 0, err.decode()[-2000:]
    assert open("trainingData/input_data_LPF50.npy", "rb").read() == single
    assert open("trainingData/last_input_data.npy", "rb").read() == single
    assert not [f for f in os.listdir("trainingData") if ".rank" in f]
