"""65 536 raw 11 x 128 windows (a corpus-sized input_data.npy holds 10^5 .. 10^6) scored with a glorot model, host memory in:
(a) one f2_cnn_score_windows call with normalize = 1 against (b) the same work as TrainAndPlotLoss ends with -
normalizeInputBatch (float64 host transpose + K3), predict_labels (second upload, scores and labels down) and the NumPy loss and
accuracy lines. Wall time per repetition (both are blocking host calls that end in a stream synchronise), mean, standard deviation,
median and min / max over two alternated passes of REPS warm repetitions each (after WARM unmeasured ones); the two results are
compared before anything is timed. Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for cfg1_latency.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.scripts.CNN import Training

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=65536)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--out")
args = ap.parse_args()

ROWS, C = 11, 128
n = args.windows
ctx = _lib.Context(0)
model = F2CNNModel.glorot(7, ROWS, C)
rng = np.random.default_rng(1)
w = np.exp(rng.normal(0.0, 1.0, (n, ROWS, C))).astype(np.float32)
y = rng.integers(0, 2, n).astype(np.uint8)
yi = y.astype(np.int64)


def new_call():
    return model.evaluate(w, y, normalize=True, ctx=ctx)


def parent_route():
    x = Training.normalizeInputBatch(w, ctx)
    scores, labels = model.predict_labels(x, ctx)
    p = np.clip(scores[np.arange(n), yi].astype(np.float64), 1e-7, 1.0)
    return float(-np.log(p).mean()), float((labels == yi).mean())


(la, aa), (lb, ab) = new_call(), parent_route()
assert aa == ab and abs(la - lb) <= 1e-12 * lb, ((la, aa), (lb, ab))


def timed(fn):
    for _ in range(args.warm):
        fn()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


# alternate the two so that neither owns the warmer half of the run
a1, b1, a2, b2 = timed(new_call), timed(parent_route), timed(new_call), timed(parent_route)


def stat(t):
    return {"mean": round(statistics.fmean(t), 3), "stdev": round(statistics.stdev(t), 3), "median": round(statistics.median(t), 3),
            "min": round(min(t), 3), "max": round(max(t), 3)}


a, b = stat(a1 + a2), stat(b1 + b2)
line = {"windows": n, "rows": ROWS, "channels": C, "reps": 2 * args.reps, "warm": args.warm, "loss": la, "accuracy": aa,
        "score_windows_ms": a, "parent_route_ms": b,
        "both_passes_ms_mean": {"score_windows": [stat(a1)["mean"], stat(a2)["mean"]], "parent_route": [stat(b1)["mean"], stat(b2)["mean"]]},
        "ratio_parent_over_score_windows": round(b["mean"] / a["mean"], 3),
        "windows_per_s": {"score_windows": round(n / a["mean"] * 1e3), "parent_route": round(n / b["mean"] * 1e3)}}
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
ctx.close()
