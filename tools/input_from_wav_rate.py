#!/usr/bin/env python3
"""`prepare input --from-wav` against the two-step route to the same training file, on one synthetic corpus.

    python3 tools/input_from_wav_rate.py [--files N] [--seed S] [--out FILE.json]

Corpus (temporary directory, tmpfs when it has room): N utterances of 1-4 s (bench.synth_utterance), every third one RIFF,
the others NIST SPHERE, split over TEST / TRAIN; a label CSV that keeps about half of the 10 ms frames inside each file's
legal range [radius*step, n - 1 - radius*step], rows of the files interleaved.

  (a) `prepare features --cutoff 50` (writes .GFB.npy + .ENV1.npy) followed by `prepare input --cutoff 50`
  (b) `prepare input --from-wav --cutoff 50`

Both as CLI calls in this process, after one untimed run of (b) (library load, tables, allocations). Prints one JSON
object: audio-s/s of (a) and (b) and their ratio, the rows of (a) against (b), and, from a further run of (b) with the
context's per-kernel timing on (f2_prof), the launches and device time of the gather (F2_K_GATHER) against the envelope
kernels (F2_K_FUSED + F2_K_SPECTRUM + F2_K_TAIL + F2_K_FILTERBANK + F2_K_ENVELOPE)."""
import argparse
import contextlib
import glob
import inspect
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from f2cnn_amd import _lib, cli, config, wavio  # noqa: E402

ENVELOPE_KERNELS = ("k_spectral_envelope", "k_utterance_spectrum", "k_tail_state", "k_erb_filterbank", "k_envelope")


def make_corpus(n_files, seed):
    from scipy.io import wavfile
    config.write_default()
    rng = np.random.default_rng(seed)
    lens, rows = {}, []
    for i in range(n_files):
        key = "{}/DR{}.S{:04d}0.SA1".format("TEST" if i % 4 == 0 else "TRAIN", 1 + i % 8, i)
        n = int(rng.integers(16000, 64001))
        os.makedirs(os.path.join("resources", "f2cnn", os.path.dirname(key)), exist_ok=True)
        w = bench.synth_utterance(seed + i, n)
        path = os.path.join("resources", "f2cnn", key + ".WAV")
        if i % 3 == 1:
            wavfile.write(path, 16000, w)
        else:
            wavio.write_sphere(path, 16000, w)
        lens[key] = n
        tt, rest = key.split("/")
        region, speaker, sentence = rest.split(".")
        frames = np.arange(800, n - 800, 160)
        for tp in frames[rng.random(frames.size) < 0.5]:
            rows.append((tt, region, speaker, sentence, "aa", int(tp)))
    rng.shuffle(rows)
    os.makedirs("trainingData", exist_ok=True)
    with open("trainingData/label_data.csv", "w") as f:
        for r in rows:
            f.write(",".join(map(str, r)) + ",0.5,0.01,1\n")
    return lens, len(rows)


def run(argv):
    t = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(argv) == 0, argv
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    need = args.files * 2.5 * 16000 * 128 * 8 * 2 * 1.5          # .GFB.npy + .ENV1.npy of (a), with room
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * need else None
    base = tempfile.mkdtemp(prefix="f2fromwav_", dir=shm)
    cwd = os.getcwd()
    os.chdir(base)
    try:
        lens, n_rows = make_corpus(args.files, args.seed)
        audio_s = sum(lens.values()) / 16000.0
        ctx = _lib.default_context()
        run(["prepare", "input", "--from-wav", "--cutoff", "50", "--input", "trainingData/warm.npy"])
        t_feat = run(["prepare", "features", "--cutoff", "50"])
        t_inp = run(["prepare", "input", "--cutoff", "50", "--input", "trainingData/two_step.npy"])
        for f in glob.glob("resources/f2cnn/*/*.npy"):
            os.remove(f)
        t_b = [run(["prepare", "input", "--from-wav", "--cutoff", "50", "--metrics", "m.json"]) for _ in range(3)]
        metrics = json.load(open("m.json"))
        a, b = np.load("trainingData/two_step.npy"), np.load("trainingData/input_data_LPF50.npy")
        err = float((np.abs(a.astype(np.float64) - b).max(axis=(1, 2)) / np.abs(a).max(axis=(1, 2))).max())
        ctx.prof_enable(True)
        run(["prepare", "input", "--from-wav", "--cutoff", "50", "--input", "trainingData/prof.npy"])
        prof = ctx.prof_get()
        ctx.prof_enable(False)
        env_ms = sum(prof.get(k, (0, 0.0))[1] for k in ENVELOPE_KERNELS)
        g_n, g_ms = prof.get("k_gather_windows", (0, 0.0))
        from f2cnn_amd.scripts.processing.InputGenerator import GenerateInputDataFromWav
        batch = inspect.signature(GenerateInputDataFromWav).parameters["batch_files"].default
        res = {
            "corpus": {"files": args.files, "audio_s": round(audio_s, 2), "windows": n_rows, "riff_files": len(range(1, args.files, 3)),
                       "lengths_s": [1, 4], "tmpfs": shm is not None},
            "a_features_s": round(t_feat, 3), "a_input_s": round(t_inp, 3),
            "a_audio_s_per_s": round(audio_s / (t_feat + t_inp), 1),
            "b_wall_s": [round(t, 3) for t in t_b], "b_audio_s_per_s": round(audio_s / min(t_b), 1),
            "b_audio_s_per_s_median": round(audio_s / sorted(t_b)[1], 1),
            "b_metrics_json": metrics,
            "ratio_b_over_a": round((t_feat + t_inp) / min(t_b), 1),
            "rows_a_vs_b_max_rel_err_per_window": err, "rows_identical": bool(np.array_equal(a, b)),
            "prof": {k: [n, round(ms, 3)] for k, (n, ms) in sorted(prof.items())},
            "batch_files": batch, "batches": -(-args.files // batch),
            "gather_launches": g_n, "gather_ms": round(g_ms, 3), "envelope_kernels_ms": round(env_ms, 3),
            "gather_share_of_device_time": round(g_ms / (g_ms + env_ms), 4) if g_ms + env_ms > 0 else None,
        }
    finally:
        os.chdir(cwd)
        shutil.rmtree(base, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
