"""`cnn noisesweep --colours`: its kernel against the float64 vector peak, and the call against the white sweep and against the only
route there was before it. Nine levels (pink, brown, speech at 20, 10 and 0 dB) of 1025 taps, 3 s utterances at 16 kHz.
(a) f2_shaped_noise_levels alone, device memory, 16 utterances: HIP-event time over INNER back-to-back calls, median over REPS, with
    the nine 1025-tap filters and with nine one-tap filters (the same launches and deviates of a 1028-sample shorter span, no tap
    walk to speak of: what is left is sigma, the deviates and the stores). FMAs per second (n * T per utterance and level) against the
    39.3 T FMA/s (78.6 TFLOP/s) float64 vector peak, for the whole call and for the difference of the two runs.
(b) One f2_eval_shaped_noise_sweep call, host memory in and labels out, one utterance and 16, a decision per frame (hop = STEP) and
    hop 16, against the white f2_eval_noise_sweep at the same K (the price of colour) and against NumPy deviates, scipy.signal.lfilter
    per level on the host and K + 1 f2_eval_batch_strided host calls. Wall time per repetition (all are blocking host calls), median
    over REPS warm repetitions (the two device routes in two alternated passes, the host route in one pass between them).
Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, json, os, socket, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for noise_sweep_timing.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.noise import ColourFIR
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--out")
args = ap.parse_args()

from scipy.signal import lfilter

C, RADIUS, STEP, FS, TAPS = 128, 5, 160, 16000, 1025
COLOURS, SNRS = ("pink", "brown", "speech"), (20.0, 10.0, 0.0)
FIRS = [ColourFIR(c, FS, TAPS) for c in COLOURS for _ in SNRS]
SNR = np.array([v for _ in COLOURS for v in SNRS])
K, N = len(FIRS), int(FS * args.seconds)
PEAK_FMA = 39.3e12
ctx = _lib.Context(0)
coefs = filters.make_erb_filters(FS, filters.centre_freqs(FS, C, 100))
h = F2CNNModel.glorot(11).handle(ctx)
stat = lambda t: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def timed(fn, warm=None):
    for _ in range(args.warm if warm is None else warm):
        fn()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


# (a) the kernel alone
B = 16
offsets = np.arange(B + 1, dtype=np.int64) * N
wave = np.ascontiguousarray(bench.synth_batch(1234, 0, B, N)).reshape(-1).astype(np.int16)
d_wave = ctx.malloc(wave.nbytes)
ctx.h2d(d_wave, wave)
d_levels = ctx.malloc(8 * (K + 1) * wave.size)
sigma = np.zeros((K + 1) * B)
e0, e1 = ctx.event(), ctx.event()
kernel = {}
for name, firs in (("taps_1025", FIRS), ("taps_1", [np.ones(1)] * K)):
    def kernel_ms():
        ctx.record(e0)
        for _ in range(args.inner):
            ctx.shaped_noise_levels(d_wave, _lib.WAVE_I16, offsets, B, SNR, firs, 7, d_levels, _lib.MEM_DEVICE, sigma=sigma)
        ctx.record(e1)
        ctx.synchronize()
        return ctx.elapsed_ms(e0, e1) / args.inner

    for _ in range(args.warm):
        kernel_ms()
    tiles = B * -(-N // _lib.SHAPED_BLOCK)
    span = -(-len(firs[0]) // 4) * 4 + _lib.SHAPED_BLOCK             # deviates a full tile stages
    kernel[name] = {"taps": len(firs[0]), "fmas": B * N * K * len(firs[0]), "deviates": K * tiles * span, "call_ms": stat([kernel_ms() for _ in range(args.reps)])}
long, short = kernel["taps_1025"], kernel["taps_1"]
walk_ms = long["call_ms"]["median"] - short["call_ms"]["median"]
for entry, ms in ((long, long["call_ms"]["median"]),):
    entry["tfma_per_s"] = round(entry["fmas"] / (ms * 1e-3) / 1e12, 3)
    entry["fraction_of_float64_vector_peak"] = round(entry["fmas"] / (ms * 1e-3) / PEAK_FMA, 4)
split = {"difference_ms": round(walk_ms, 4), "note": "taps_1025 minus taps_1: the tap walk and the deviates of the 1024 samples more "
         "that a tile's span holds at 1025 taps", "ns_per_deviate_from_taps_1": round(short["call_ms"]["median"] * 1e6 / short["deviates"], 4)}
split["deviates_ms_at_1025_taps_from_that_rate"] = round(split["ns_per_deviate_from_taps_1"] * long["deviates"] * 1e-6, 4)
split["tap_walk_ms"] = round(long["call_ms"]["median"] - split["deviates_ms_at_1025_taps_from_that_rate"], 4)
split["tap_walk_tfma_per_s"] = round(long["fmas"] / (split["tap_walk_ms"] * 1e-3) / 1e12, 3)
split["tap_walk_fraction_of_float64_vector_peak"] = round(long["fmas"] / (split["tap_walk_ms"] * 1e-3) / PEAK_FMA, 4)
ctx.free(d_wave)
ctx.free(d_levels)

# (b) the call
cases = {}
for B in (1, 16):
    wave = np.ascontiguousarray(bench.synth_batch(1234, 0, B, N)).reshape(-1).astype(np.int16)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    for hop in (STEP, 16):
        nw = B * _lib.strided_window_count(N, RADIUS, STEP, hop)
        labels = np.empty((K + 1) * nw, np.uint8)
        rng = np.random.default_rng(7)

        def coloured():
            ctx.eval_shaped_noise_sweep(h, wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, SNR, FIRS,
                                        7, None, None, labels, _lib.MEM_HOST)

        def white():
            ctx.eval_noise_sweep(h, wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, SNR, 7, None, None,
                                 labels, _lib.MEM_HOST)

        def host_route():
            x = wave.astype(np.float64).reshape(B, N)
            rms = np.sqrt(np.mean(np.square(x), axis=1, keepdims=True))
            for k in range(K + 1):
                if k < K:
                    z = lfilter(FIRS[k], 1.0, rng.standard_normal((B, N + TAPS - 1)), axis=1)[:, TAPS - 1:]
                    w, dt = np.ascontiguousarray(x + rms / 10 ** (SNR[k] / 10) * z).reshape(-1), _lib.WAVE_F64
                else:
                    w, dt = wave, _lib.WAVE_I16
                ctx.eval_batch_strided(h, w, dt, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, None,
                                       labels[k * nw:(k + 1) * nw], _lib.MEM_HOST)

        # the device routes alternate in two passes; the host route, seconds per call at 16 utterances, runs one pass between them
        a1, b1, c1, a2, b2 = timed(coloured), timed(white), timed(host_route, warm=1), timed(coloured), timed(white)
        a, b, c = stat(a1 + a2), stat(b1 + b2), stat(c1)
        cases["B{}_hop{}".format(B, hop)] = {
            "utterances": B, "hop": hop, "windows_per_level": nw, "coloured_sweep_ms": a, "white_sweep_ms": b,
            "numpy_lfilter_then_strided_calls_ms": c, "ratio_coloured_over_white": round(a["median"] / b["median"], 3),
            "ratio_host_route_over_coloured": round(c["median"] / a["median"], 3)}

line = {"box": socket.gethostname(), "utterance_samples": N, "levels": K, "colours": list(COLOURS), "snr_db": list(SNRS), "taps": TAPS,
        "reps": args.reps, "warm": args.warm, "memory": "device for the kernel, host for the routes",
        "f2_shaped_noise_levels": {"utterances": 16, "calls_per_measurement": args.inner, "peak_fma_per_s": PEAK_FMA, "runs": kernel,
                                   "split": split},
        "cases": cases}
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
ctx.close()
