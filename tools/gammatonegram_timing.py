"""256 utterances of 3 s (int16, host memory), 128 channels, pictures of 1600 columns:
(a) one f2_gammatonegram_batch call to host `levels` against (b) the only route there was before it -
f2_filterbank_envelope_fused to host memory (8 * C * samples bytes over the link) followed by the pooling and LogNorm levels in
NumPy. Wall time per repetition (both end in a stream synchronise), mean, standard deviation, median and min / max over two
alternated passes of REPS warm repetitions each (after WARM unmeasured ones); the two results are compared before anything is
timed. Also the HIP-event time of the two picture kernels alone (f2_envelope_picture on envelopes resident in device memory,
pooled and levels to device memory) and the fraction of the HBM peak that 8 * C * samples bytes in that time come to.
Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for cfg1_latency.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters

ap = argparse.ArgumentParser()
ap.add_argument("--utterances", type=int, default=256)
ap.add_argument("--samples", type=int, default=48000)
ap.add_argument("--width", type=int, default=1600)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--out")
args = ap.parse_args()

C, FS, HBM_PEAK = 128, 16000, 8e12
B, n, W = args.utterances, args.samples, args.width
ctx = _lib.Context(0)
coefs = np.ascontiguousarray(filters.make_erb_filters(FS, filters.centre_freqs(FS, C, 100)), dtype=np.float64)
rng = np.random.default_rng(16)
wave = np.clip(np.round(rng.standard_normal(B * n) * 3000.0), -32768, 32767).astype(np.int16)
offsets = np.arange(B + 1, dtype=np.int64) * n
levels = np.zeros((B, C, W), np.uint8)
env = np.empty(C * B * n)
x = np.arange(W, dtype=np.int64)
lo, hi = x * n // W, (x + 1) * n // W
hi = np.where(hi == lo, lo + 1, hi)


def new_call():
    ctx.gammatonegram_batch(wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, None, W, 0, None, levels, _lib.MEM_HOST)
    return levels


def numpy_picture(e):
    """mean per column and LogNorm levels of the (B, C, n) envelopes, as the definition in include/f2cnn_hip.h"""
    if n % W == 0:
        pooled = e.reshape(B, C, W, n // W).mean(axis=3)
    else:
        pooled = np.add.reduceat(e.reshape(B, C, n), lo, axis=2) / (hi - lo)      # (bins tile the row when n >= W)
    out = np.zeros(pooled.shape, np.uint8)
    for b in range(B):
        p = pooled[b]
        pos = p > 0
        if pos.any():
            lmin, lmax = np.log(p[pos].min()), np.log(p[pos].max())
            t = (np.log(p[pos]) - lmin) / (lmax - lmin) if lmax > lmin else np.zeros(pos.sum())
            out[b][pos] = 1 + (254.0 * t + 0.5).astype(np.int64)
    return out


def parent_route():
    ctx.filterbank_envelope_fused(wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, env, None, _lib.MEM_HOST)
    return numpy_picture(env)


assert n >= W, "the NumPy route of this tool pools whole bins"
la, lb = new_call().copy(), parent_route()
diff = np.abs(la.astype(np.int64) - lb.astype(np.int64))
assert diff.max() <= 1, diff.max()


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

# the picture kernels alone: envelopes resident in device memory
d_wave, d_env = ctx.malloc(wave.nbytes), ctx.malloc(env.nbytes)
d_pooled, d_levels = ctx.malloc(8 * B * C * W), ctx.malloc(B * C * W)
ctx.h2d(d_wave, wave)
ctx.filterbank_envelope_fused(d_wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, d_env, None, _lib.MEM_DEVICE)
ctx.synchronize()
e0, e1 = ctx.event(), ctx.event()
kernel_ms = []
for rep in range(args.warm + 2 * args.reps):
    ctx.record(e0)
    ctx.envelope_picture(d_env, offsets, B, C, None, W, 0, d_pooled, d_levels, _lib.MEM_DEVICE)
    ctx.record(e1)
    if rep >= args.warm:
        kernel_ms.append(ctx.elapsed_ms(e0, e1))
dev_levels = np.zeros_like(levels)
ctx.d2h(dev_levels, d_levels)
assert np.array_equal(dev_levels, la)
for p in (d_wave, d_env, d_pooled, d_levels):
    ctx.free(p)


def stat(t):
    return {"mean": round(statistics.fmean(t), 3), "stdev": round(statistics.stdev(t), 3), "median": round(statistics.median(t), 3),
            "min": round(min(t), 3), "max": round(max(t), 3)}


a, b, k = stat(a1 + a2), stat(b1 + b2), stat(kernel_ms)
env_bytes = 8 * C * B * n
line = {"utterances": B, "samples": n, "channels": C, "width": W, "pool": "mean", "reps": 2 * args.reps, "warm": args.warm,
        "levels_differing_by_one": int((diff == 1).sum()), "pixels": int(diff.size),
        "gammatonegram_batch_ms": a, "fused_to_host_then_numpy_ms": b,
        "both_passes_ms_mean": {"gammatonegram_batch": [stat(a1)["mean"], stat(a2)["mean"]],
                                "fused_to_host_then_numpy": [stat(b1)["mean"], stat(b2)["mean"]]},
        "ratio_parent_over_gammatonegram_batch": round(b["mean"] / a["mean"], 3),
        "audio_s_per_s": {"gammatonegram_batch": round(B * n / FS / a["mean"] * 1e3, 1),
                          "fused_to_host_then_numpy": round(B * n / FS / b["mean"] * 1e3, 1)},
        "bytes_to_host": {"gammatonegram_batch": int(levels.nbytes), "fused_to_host_then_numpy": env_bytes},
        "picture_kernels_event_ms": k, "envelope_bytes": env_bytes,
        "picture_kernels_fraction_of_hbm_peak": round(env_bytes / (k["mean"] * 1e-3) / HBM_PEAK, 4), "hbm_peak_bytes_per_s": HBM_PEAK}
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
ctx.close()
