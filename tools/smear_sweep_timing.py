"""`cnn smearsweep` against the route there was before it, and its kernel against the HBM and the float64 vector peaks.
Levels: channel interaction of 0.5 / 1 / 2 / 4 ERB, an 8-band vocoder, and the sharp level; 3 s utterances, 128 channels.
(a) One f2_eval_smear_sweep call, host memory in, labels out: 1 and 16 utterances, at hop = STEP and at hop 16.
(b) The host route: f2_filterbank_envelope_fused with the envelopes to the host, `W @ env` in NumPy per level and utterance, then
    per level f2_gather_windows(normalize = 1) per utterance and one f2_cnn_forward, all from host memory.
    Wall time per repetition, median over two alternated passes of REPS warm repetitions each.
(c) f2_channel_mix_levels alone on 16 x 3 s x 128 channels in device memory: HIP-event time over INNER back-to-back device calls,
    median over REPS - all five matrices in one call, and each alone - as a fraction of the 8 TB/s HBM peak for the
    8 C total (K + 2) bytes it must move, and as FMAs per second (the contract's: one per weight inside a row's support and
    sample; `walked` adds the zero weights of the tiles' spans) against the 39.3 T FMA/s float64 vector peak.
Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for noise_sweep_timing.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib, smear
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=5, help="repetitions per pass of the host route (b)")
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--out")
args = ap.parse_args()

C, RADIUS, STEP = 128, 5, 160
R = 2 * RADIUS + 1
SPREADS, BANDS = (0.5, 1.0, 2.0, 4.0), (8,)
N = int(16000 * args.seconds)
HOST, DEV = _lib.MEM_HOST, _lib.MEM_DEVICE
FMA_PEAK = 39.3e12
ctx = _lib.Context(0)
freqs = filters.centre_freqs(16000, C, 100)
coefs = np.ascontiguousarray(filters.make_erb_filters(16000, freqs))
MIX = np.stack([smear.SmearMatrix(freqs, v) for v in SPREADS] + [smear.BandMatrix(C, v) for v in BANDS])
NAMES = ["{:g}ERB".format(v) for v in SPREADS] + ["{}bands".format(v) for v in BANDS]
K = len(MIX)
h = F2CNNModel.glorot(11).handle(ctx)
TS, TC = _lib.SMEAR_TILE_SAMPLES, _lib.SMEAR_TILE_CHANNELS


def timed(fn, reps):
    for _ in range(args.warm):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def fmas_per_column(W):
    """(the contract's FMAs, the FMAs the kernel walks) per sample column"""
    useful = walked = 0
    for c0 in range(0, C, TC):
        rows = W[c0:c0 + TC]
        for row in rows:
            nz = np.flatnonzero(row)
            useful += int(nz[-1] - nz[0] + 1) if len(nz) else 0
        cols = np.flatnonzero(rows.any(axis=0))
        walked += TC * int(cols[-1] - cols[0] + 1) if len(cols) else 0
    return useful, walked


stat = lambda t: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
cases = {}
for B in (1, 16):
    wave = np.ascontiguousarray(bench.synth_batch(1234, 0, B, N)).reshape(-1).astype(np.int16)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    for hop in (STEP, 16):
        per = _lib.strided_window_count(N, RADIUS, STEP, hop)
        nw = B * per
        labels = np.zeros((K + 1) * nw, np.uint8)
        labels_b = np.zeros((K + 1) * nw, np.uint8)
        centers = (RADIUS * STEP + hop * np.arange(per)).astype(np.int64)
        env = np.empty(C * B * N)
        win = np.empty((nw, R, C), np.float32)
        scores = np.empty((nw, 2), np.float32)

        def sweep():
            ctx.eval_smear_sweep(h, wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, MIX, None, None,
                                 labels, HOST)

        def host_route():
            ctx.filterbank_envelope_fused(wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, env, None, HOST)
            blocks = env.reshape(B, C, N)
            for l in range(K + 1):
                for b in range(B):
                    lev = blocks[b] if l == K else np.ascontiguousarray(MIX[l] @ blocks[b])
                    ctx.gather_windows(lev, C, N, centers, per, RADIUS, STEP, True, win[b * per:(b + 1) * per], HOST)
                ctx.cnn_forward(h, win, nw, scores, labels_b[l * nw:(l + 1) * nw], HOST)

        # alternate the two so that neither owns the warmer half of the run; each figure is the median over both of its passes
        a1, b1, a2, b2 = timed(sweep, args.reps), timed(host_route, args.host_reps), timed(sweep, args.reps), timed(host_route, args.host_reps)
        a, b = stat(a1 + a2), stat(b1 + b2)
        cases["B{}_hop{}".format(B, hop)] = {
            "utterances": B, "hop": hop, "windows_per_level": nw, "sweep_ms": a, "host_route_ms": b,
            "passes_ms_median": {"sweep": [stat(a1)["median"], stat(a2)["median"]], "host_route": [stat(b1)["median"], stat(b2)["median"]]},
            "ratio_host_route_over_sweep": round(b["median"] / a["median"], 3),
            "labels_equal": bool(np.array_equal(labels, labels_b)), "labels_differing": int((labels != labels_b).sum())}

# (c) the kernel alone
B = 16
total = B * N
offsets = np.arange(B + 1, dtype=np.int64) * N
env = np.abs(np.random.default_rng(3).standard_normal(C * total)) + 0.1
held = []
d_env = ctx.malloc(env.nbytes)
held.append(d_env)
ctx.h2d(d_env, env)
d_levels = ctx.malloc((K + 1) * env.nbytes)
held.append(d_levels)
e0, e1 = ctx.event(), ctx.event()


def kernel_stats(mix):
    def once():
        ctx.record(e0)
        for _ in range(args.inner):
            ctx.channel_mix_levels(d_env, offsets, B, C, mix, d_levels, DEV)
        ctx.record(e1)
        ctx.synchronize()
        return ctx.elapsed_ms(e0, e1) / args.inner
    for _ in range(args.warm):
        once()
    ks = stat([once() for _ in range(args.reps)])
    k = len(mix)
    counts = [fmas_per_column(W) for W in mix]
    useful, walked = sum(u for u, _ in counts) * total, sum(w for _, w in counts) * total
    must_move = 8 * (k + 2) * C * total
    sec = ks["median"] * 1e-3
    return {"levels": k, "call_ms": ks, "bytes_moved": must_move, "gbytes_per_s": round(must_move / sec / 1e9, 1),
            "fraction_of_8TBps": round(must_move / sec / 8e12, 4), "fmas": useful, "fmas_walked": walked,
            "tfma_per_s": round(useful / sec / 1e12, 2), "tfma_per_s_walked": round(walked / sec / 1e12, 2),
            "fraction_of_fp64_vector_peak": round(useful / sec / FMA_PEAK, 4), "fraction_of_fp64_vector_peak_walked": round(walked / sec / FMA_PEAK, 4)}


kernel = {"utterances": B, "channels": C, "samples": total, "calls_per_measurement": args.inner, "fp64_vector_peak_fma_per_s": FMA_PEAK,
          "fmas_per_column": {n: fmas_per_column(W)[0] for n, W in zip(NAMES, MIX)},
          "fmas_walked_per_column": {n: fmas_per_column(W)[1] for n, W in zip(NAMES, MIX)},
          "all": kernel_stats(MIX), "each": {n: kernel_stats(MIX[l:l + 1]) for l, n in enumerate(NAMES)}}
line = {"utterance_samples": N, "levels": NAMES + ["sharp"], "reps": 2 * args.reps, "host_route_reps": 2 * args.host_reps, "warm": args.warm,
        "memory": "host in, labels out", "cases": cases, "k_channel_mix_levels": kernel}
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
for p in held:
    ctx.free(p)
ctx.close()
