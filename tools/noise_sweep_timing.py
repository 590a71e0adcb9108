"""One 3 s utterance at K = 5 noise levels and clean, one decision per frame (hop = STEP), host memory in and out:
(a) one f2_eval_noise_sweep call against (b) the same work as `cnn evalnoise` does it - NumPy noise on the host (Evaluating.
add_gaussian_noise) and six one-utterance f2_eval_batch_strided host calls, five float64 and the clean int16 one. Wall time per
repetition with the stream synchronised inside the timed region (both are blocking host calls; a synchronise follows anyway),
median over two alternated passes of REPS warm repetitions (each after WARM unmeasured ones). Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for cfg1_latency.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.scripts.CNN import Evaluating
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--out")
args = ap.parse_args()
assert args.reps >= 20

C, RADIUS, STEP = 128, 5, 160
SNR = np.array([20.0, 10.0, 5.0, 0.0, -3.0])
K, N, HOP = len(SNR), int(16000 * args.seconds), STEP
ctx = _lib.Context(0)
coefs = filters.make_erb_filters(16000, filters.centre_freqs(16000, C, 100))
h = F2CNNModel.glorot(11).handle(ctx)
wave = np.ascontiguousarray(bench.synth_batch(1234, 0, 1, N)).reshape(-1).astype(np.int16)
offsets = np.array([0, N], np.int64)
nw = _lib.strided_window_count(N, RADIUS, STEP, HOP)
labels = np.empty((K + 1) * nw, np.uint8)
rng = np.random.default_rng(7)


def sweep():
    ctx.eval_noise_sweep(h, wave, _lib.WAVE_I16, offsets, coefs, 1, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, HOP, SNR, 7, None, None,
                         labels, _lib.MEM_HOST)
    ctx.synchronize()


def one_by_one():
    for k in range(K + 1):
        w, dt = (Evaluating.add_gaussian_noise(wave, SNR[k], rng), _lib.WAVE_F64) if k < K else (wave, _lib.WAVE_I16)
        ctx.eval_batch_strided(h, w, dt, offsets, coefs, 1, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, HOP, None, labels[k * nw:(k + 1) * nw],
                               _lib.MEM_HOST)
    ctx.synchronize()


def timed(fn):
    for _ in range(args.warm):
        fn()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


# alternate the two so that neither owns the warmer half of the run; each figure is the median over both of its passes
a1, b1, a2, b2 = timed(sweep), timed(one_by_one), timed(sweep), timed(one_by_one)
stat = lambda t: (statistics.median(t), min(t), max(t))
a, b = stat(a1 + a2), stat(b1 + b2)
a1, a2, b1, b2 = stat(a1), stat(a2), stat(b1), stat(b2)
line = {"utterance_samples": N, "levels": K, "hop": HOP, "windows_per_level": nw, "reps": 2 * args.reps, "warm": args.warm,
        "sweep_ms_median": round(a[0], 4), "sweep_ms_min_max": [round(a[1], 4), round(a[2], 4)],
        "one_by_one_ms_median": round(b[0], 4), "one_by_one_ms_min_max": [round(b[1], 4), round(b[2], 4)],
        "both_passes_ms_median": {"sweep": [round(a1[0], 4), round(a2[0], 4)], "one_by_one": [round(b1[0], 4), round(b2[0], 4)]},
        "ratio_one_by_one_over_sweep": round(b[0] / a[0], 3)}
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
ctx.close()
