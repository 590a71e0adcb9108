"""`cnn reverbsweep` against the only route there was before it, and its kernel against the float64 vector peak. T60 = 0.1, 0.2,
0.4, 0.8 and 1.6 s (1600 .. 25 600 taps at 16 kHz), one decision per frame (hop = STEP), one 3 s utterance and 16 of them.
(a) One f2_eval_reverb_sweep call, host memory in and labels out, against scipy.signal.fftconvolve per level on the host followed
    by K + 1 f2_eval_batch_strided host calls (five float64 batches and the dry int16 one), and against ONE plain strided call on
    the dry batch (what the five extra levels cost). Wall time per repetition (all are blocking host calls), median over two
    alternated passes of REPS warm repetitions each.
(b) f2_reverb_levels alone, device memory: HIP-event time over INNER back-to-back calls, median over REPS, for each response on
    its own and for all five, as FMAs per second (the sum_k min(k + 1, T) terms of the definition) against the 39.3 T FMA/s
    (78.6 TFLOP/s) float64 vector peak.
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
from f2cnn_amd.reverb import SyntheticRIR
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--out")
args = ap.parse_args()
assert args.reps >= 20

from scipy.signal import fftconvolve

C, RADIUS, STEP, FS = 128, 5, 160, 16000
T60 = (0.1, 0.2, 0.4, 0.8, 1.6)
RIRS = [SyntheticRIR(t, FS, seed=7, level=l) for l, t in enumerate(T60)]
K, N, HOP = len(RIRS), int(FS * args.seconds), STEP
PEAK_FMA = 39.3e12
ctx = _lib.Context(0)
coefs = filters.make_erb_filters(FS, filters.centre_freqs(FS, C, 100))
h = F2CNNModel.glorot(11).handle(ctx)


def timed(fn):
    for _ in range(args.warm):
        fn()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def fmas(n, taps):
    """terms of sum_{t <= min(k, T - 1)} over k < n"""
    m = min(n, taps)
    return m * (m + 1) // 2 + (n - m) * taps


stat = lambda t: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
cases = {}
for B in (1, 16):
    wave = np.ascontiguousarray(bench.synth_batch(1234, 0, B, N)).reshape(-1).astype(np.int16)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    nw = B * _lib.strided_window_count(N, RADIUS, STEP, HOP)
    labels = np.empty((K + 1) * nw, np.uint8)

    def sweep():
        ctx.eval_reverb_sweep(h, wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, HOP, RIRS, None, None,
                              labels, _lib.MEM_HOST)
        ctx.synchronize()

    def host_route():
        x = wave.astype(np.float64).reshape(B, N)
        for k in range(K + 1):
            if k < K:
                w, dt = np.ascontiguousarray(fftconvolve(x, RIRS[k][None, :], axes=1)[:, :N]).reshape(-1), _lib.WAVE_F64
            else:
                w, dt = wave, _lib.WAVE_I16
            ctx.eval_batch_strided(h, w, dt, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, HOP, None,
                                   labels[k * nw:(k + 1) * nw], _lib.MEM_HOST)
        ctx.synchronize()

    def dry_only():
        ctx.eval_batch_strided(h, wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, HOP, None, labels[:nw],
                               _lib.MEM_HOST)
        ctx.synchronize()

    # alternate the routes so that none owns the warmer part of the run; each figure is the median over both of its passes
    a1, b1, c1, a2, b2, c2 = timed(sweep), timed(host_route), timed(dry_only), timed(sweep), timed(host_route), timed(dry_only)
    a, b, c = stat(a1 + a2), stat(b1 + b2), stat(c1 + c2)
    cases["B{}".format(B)] = {
        "utterances": B, "hop": HOP, "windows_per_level": nw, "sweep_ms": a, "fftconvolve_then_strided_calls_ms": b, "dry_strided_call_ms": c,
        "passes_ms_median": {"sweep": [stat(a1)["median"], stat(a2)["median"]], "host_route": [stat(b1)["median"], stat(b2)["median"]],
                             "dry": [stat(c1)["median"], stat(c2)["median"]]},
        "ratio_host_route_over_sweep": round(b["median"] / a["median"], 3), "ratio_sweep_over_dry": round(a["median"] / c["median"], 3)}

# (b) the kernel alone
B = 16
offsets = np.arange(B + 1, dtype=np.int64) * N
wave = np.ascontiguousarray(bench.synth_batch(1234, 0, B, N)).reshape(-1).astype(np.int16)
d_wave = ctx.malloc(wave.nbytes)
ctx.h2d(d_wave, wave)
d_levels = ctx.malloc(8 * (K + 1) * wave.size)
e0, e1 = ctx.event(), ctx.event()
kernel = {}
for name, rirs in [("T60_{:g}s".format(t), [r]) for t, r in zip(T60, RIRS)] + [("all_five", RIRS)]:
    def kernel_ms():
        ctx.record(e0)
        for _ in range(args.inner):
            ctx.reverb_levels(d_wave, _lib.WAVE_I16, offsets, B, rirs, d_levels, _lib.MEM_DEVICE)
        ctx.record(e1)
        ctx.synchronize()
        return ctx.elapsed_ms(e0, e1) / args.inner

    for _ in range(args.warm):
        kernel_ms()
    ks = stat([kernel_ms() for _ in range(args.reps)])
    work = B * sum(fmas(N, len(r)) for r in rirs)
    kernel[name] = {"taps": [len(r) for r in rirs], "fmas": work, "call_ms": ks, "tfma_per_s": round(work / (ks["median"] * 1e-3) / 1e12, 3),
                    "fraction_of_float64_vector_peak": round(work / (ks["median"] * 1e-3) / PEAK_FMA, 4)}
line = {"utterance_samples": N, "t60_s": list(T60), "taps": [len(r) for r in RIRS], "reps": 2 * args.reps, "warm": args.warm,
        "memory": "host for the routes, device for the kernel", "cases": cases,
        "f2_reverb_levels": {"utterances": B, "calls_per_measurement": args.inner, "peak_fma_per_s": PEAK_FMA, "responses": kernel}}
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
ctx.free(d_wave)
ctx.free(d_levels)
ctx.close()
