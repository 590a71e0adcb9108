"""`cnn lpfsweep` against the route it replaces, and its kernel against the HBM peak. Everything resident in device memory.
(a) One f2_eval_cutoff_sweep call (K = 5 cutoffs and the unfiltered level) against K + 1 calls of f2_eval_batch_strided with lpf /
    cutoff_hz set (the last one unfiltered): one 3 s utterance and 16 utterances of 3 s, at hop = STEP and at hop 16. Wall time per
    repetition (both routes end in a wait for the stream), median over two alternated passes of REPS warm repetitions each.
(b) f2_lowpass_levels alone on 16 x 3 s x 128 channels: HIP-event time over INNER back-to-back device calls, median over REPS, as a
    fraction of the 8 TB/s HBM peak for the 8 * (K + 2) bytes per sample it must move.
Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for noise_sweep_timing.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out")
args = ap.parse_args()
assert args.reps >= 20

C, RADIUS, STEP = 128, 5, 160
CUTOFFS = np.array([5.0, 10.0, 20.0, 50.0, 100.0])
K, N = len(CUTOFFS), int(16000 * args.seconds)
DEV = _lib.MEM_DEVICE
ctx = _lib.Context(0)
coefs = filters.make_erb_filters(16000, filters.centre_freqs(16000, C, 100))
h = F2CNNModel.glorot(11).handle(ctx)
held = []


def on_device(a):
    p = ctx.malloc(max(a.nbytes, 8))
    ctx.h2d(p, a)
    held.append(p)
    return p


def timed(fn):
    for _ in range(args.warm):
        fn()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


stat = lambda t: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
cases = {}
for B in (1, 16):
    wave = np.ascontiguousarray(bench.synth_batch(1234, 0, B, N)).reshape(-1).astype(np.int16)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    d_wave = on_device(wave)
    for hop in (STEP, 16):
        nw = B * _lib.strided_window_count(N, RADIUS, STEP, hop)
        d_labels = on_device(np.zeros((K + 1) * nw, np.uint8))

        def sweep():
            ctx.eval_cutoff_sweep(h, d_wave, _lib.WAVE_I16, offsets, coefs, B, C, _lib.FFT_F32, RADIUS, STEP, hop, CUTOFFS, None, None,
                                  d_labels, DEV)
            ctx.synchronize()

        def one_by_one():
            for k in range(K + 1):
                ctx.eval_batch_strided(h, d_wave, _lib.WAVE_I16, offsets, coefs, B, C, k < K, CUTOFFS[k] if k < K else 0.0, _lib.FFT_F32,
                                       RADIUS, STEP, hop, None, d_labels + k * nw, DEV)
            ctx.synchronize()

        # alternate the two so that neither owns the warmer half of the run; each figure is the median over both of its passes
        a1, b1, a2, b2 = timed(sweep), timed(one_by_one), timed(sweep), timed(one_by_one)
        a, b = stat(a1 + a2), stat(b1 + b2)
        cases["B{}_hop{}".format(B, hop)] = {
            "utterances": B, "hop": hop, "windows_per_level": nw, "sweep_ms": a, "one_by_one_ms": b,
            "passes_ms_median": {"sweep": [stat(a1)["median"], stat(a2)["median"]], "one_by_one": [stat(b1)["median"], stat(b2)["median"]]},
            "ratio_one_by_one_over_sweep": round(b["median"] / a["median"], 3)}

# (b) the kernel alone
B = 16
total = B * N
offsets = np.arange(B + 1, dtype=np.int64) * N
env = np.abs(np.random.default_rng(3).standard_normal(C * total)) + 0.1
d_env = on_device(env)
d_levels = ctx.malloc((K + 1) * env.nbytes)
held.append(d_levels)
e0, e1 = ctx.event(), ctx.event()


def kernel_ms():
    ctx.record(e0)
    for _ in range(args.inner):
        ctx.lowpass_levels(d_env, offsets, B, C, CUTOFFS, d_levels, DEV)
    ctx.record(e1)
    ctx.synchronize()
    return ctx.elapsed_ms(e0, e1) / args.inner


for _ in range(args.warm):
    kernel_ms()
t = [kernel_ms() for _ in range(args.reps)]
must_move = 8 * (K + 2) * C * total
ks = stat(t)
kernel = {"utterances": B, "channels": C, "samples": total, "cutoffs": K, "bytes_moved": must_move, "calls_per_measurement": args.inner,
          "call_ms": ks, "gbytes_per_s": round(must_move / (ks["median"] * 1e-3) / 1e9, 1),
          "fraction_of_8TBps": round(must_move / (ks["median"] * 1e-3) / 8e12, 4)}
line = {"utterance_samples": N, "cutoffs_hz": CUTOFFS.tolist(), "reps": 2 * args.reps, "warm": args.warm, "memory": "device",
        "cases": cases, "k_lowpass_levels": kernel}
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
for p in held:
    ctx.free(p)
ctx.close()
