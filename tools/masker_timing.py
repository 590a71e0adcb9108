"""Recorded maskers (`cnn noisesweep --maskers`, `cnn train --augment-maskers`): what the kernels and the calls cost beside what the
library had before them. Nine levels (three recordings of 10 s at 20, 10 and 0 dB), 3 s utterances at 16 kHz.
(a) f2_masker_levels alone, device memory, 16 utterances: HIP-event time over INNER back-to-back calls, median over REPS, beside
    f2_shaped_noise_levels with nine one-tap filters [1.0] at the same K - the stateless call that returns the white sweep's bits (the
    white sweep's own two kernels have no stateless entry). The bytes the masker call moves - the wave once per grid row, one read of
    the segment for the sums and one for the mix per level, (K + 1) float64 stores per sample - against the 8 TB/s HBM peak.
(b) One f2_eval_masker_sweep call, host memory in and labels out, one utterance and 16, a decision per frame (hop = STEP) and hop 16,
    against the white f2_eval_noise_sweep at the same K. Wall time per repetition (blocking host calls), median over REPS warm
    repetitions, the two routes in two alternated passes.
(c) Trainer.render with a masker level per file against Trainer.render with a white noise level per file, the same number of levels,
    --utterances files of 3 s with --centres windows each: host clock around work that ends in a device synchronise, median of 3, the
    two cases alternated, two passes.
Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, json, os, socket, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--utterances", type=int, default=400)
ap.add_argument("--centres", type=int, default=164)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--out")
args = ap.parse_args()

C, RADIUS, STEP, FS = 128, 5, 160, 16000
SNRS = (20.0, 10.0, 0.0)
MASKERS = [np.random.default_rng([5, r]).standard_normal(10 * FS) * 2000.0 for r in range(3)]
MASKER_OF = [r for r in range(len(MASKERS)) for _ in SNRS]
SNR = np.array([v for _ in MASKERS for v in SNRS])
K, N = len(SNR), int(FS * args.seconds)
PEAK_HBM = 8.0e12
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


# (a) the kernels alone
B = 16
offsets = np.arange(B + 1, dtype=np.int64) * N
wave = np.ascontiguousarray(bench.synth_batch(1234, 0, B, N)).reshape(-1).astype(np.int16)
d_wave = ctx.malloc(wave.nbytes)
ctx.h2d(d_wave, wave)
d_levels = ctx.malloc(8 * (K + 1) * wave.size)
sigma = np.zeros((K + 1) * B)
e0, e1 = ctx.event(), ctx.event()
ONE_TAP = [np.ones(1)] * K


def event_ms(call):
    def once():
        ctx.record(e0)
        for _ in range(args.inner):
            call()
        ctx.record(e1)
        ctx.synchronize()
        return ctx.elapsed_ms(e0, e1) / args.inner
    for _ in range(args.warm):
        once()
    return [once() for _ in range(args.reps)]


masker_call = lambda: ctx.masker_levels(d_wave, _lib.WAVE_I16, offsets, B, SNR, MASKERS, MASKER_OF, 7, d_levels, _lib.MEM_DEVICE)
white_call = lambda: ctx.shaped_noise_levels(d_wave, _lib.WAVE_I16, offsets, B, SNR, ONE_TAP, 7, d_levels, _lib.MEM_DEVICE, sigma=sigma)
m1, w1, m2, w2 = event_ms(masker_call), event_ms(white_call), event_ms(masker_call), event_ms(white_call)
moved = B * N * (2 * (K + 1) + 2 + 8 * (K + 1) + 2 * 8 * K)        # int16 wave per grid row and for sigma, stores, two segment reads per level
upload = 8 * sum(len(m) for m in MASKERS)
levels = {"utterances": B, "calls_per_measurement": args.inner, "masker_levels_call_ms": stat(m1 + m2),
          "white_one_tap_shaped_levels_call_ms": stat(w1 + w2), "bytes_moved_by_the_kernels": moved,
          "bytes_of_recordings_uploaded_per_call": upload, "peak_hbm_bytes_per_s": PEAK_HBM,
          "note": "the masker call also uploads its recordings (host -> device) inside the timed span"}
levels["ratio_masker_over_white"] = round(levels["masker_levels_call_ms"]["median"] / levels["white_one_tap_shaped_levels_call_ms"]["median"], 3)
levels["fraction_of_hbm_peak_of_the_whole_call"] = round(moved / (levels["masker_levels_call_ms"]["median"] * 1e-3) / PEAK_HBM, 4)
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

        def masked():
            ctx.eval_masker_sweep(h, wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, SNR, MASKERS,
                                  MASKER_OF, 7, None, None, labels, _lib.MEM_HOST)

        def white():
            ctx.eval_noise_sweep(h, wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP, hop, SNR, 7, None, None,
                                 labels, _lib.MEM_HOST)

        a1, b1, a2, b2 = timed(masked), timed(white), timed(masked), timed(white)
        a, b = stat(a1 + a2), stat(b1 + b2)
        cases["B{}_hop{}".format(B, hop)] = {"utterances": B, "hop": hop, "windows_per_level": nw, "masker_sweep_ms": a, "white_sweep_ms": b,
                                             "ratio_masker_over_white": round(a["median"] / b["median"], 3)}

# (c) the render
from f2cnn_amd.scripts.CNN import Training
from f2cnn_amd.trainer import Trainer
seed = 3
rng = np.random.default_rng(seed)
reach = RADIUS * STEP
waves = [(rng.standard_normal(N) * 3000).astype(np.int16) for _ in range(args.utterances)]
centres = [np.linspace(reach, N - 1 - reach, args.centres).astype(np.int64) for _ in range(args.utterances)]
signs = [rng.integers(0, 2, args.centres).astype(np.uint8) for _ in range(args.utterances)]
coefs64 = np.ascontiguousarray(coefs, dtype=np.float64)
trainer = Trainer(F2CNNModel.glorot(seed, 2 * RADIUS + 1, C), lr=1e-4, decay=1e-6, drop=Training.DROPOUT, seed=seed, ctx=ctx)
trainer.set_waves(waves, centres, signs, coefs64, RADIUS, STEP, group=Training.RENDER_GROUP)
draw_rng = np.random.default_rng([seed, Training.MASKER_STREAM])
draws = [Training.draw_epoch_maskers(draw_rng, K, args.utterances) for _ in range(3 * args.passes + 1)]      # the same for both cases


def render_timed(fn):
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return time.perf_counter() - t0


render_cases = {"render_white": lambda d: trainer.render(list(SNR), d[0], d[1]),
                "render_masked": lambda d: trainer.render(maskers=MASKERS, masker_of=MASKER_OF, masker_snrs=list(SNR), masker_level_of=d[0], seed=d[1])}
for fn in render_cases.values():
    fn(draws[0])
ctx.synchronize()
passes = []
for p in range(args.passes):
    got = {k: [] for k in render_cases}
    for r in range(3):
        for k, fn in render_cases.items():                                  # alternating
            got[k].append(render_timed(lambda: fn(draws[1 + 3 * p + r])))
    passes.append({k: {"host_s": [round(v, 5) for v in t], "host_median_s": round(statistics.median(t), 5)} for k, t in got.items()})
trainer.close()
render = {"utterances": args.utterances, "centres": args.centres, "windows": args.utterances * args.centres, "group": Training.RENDER_GROUP,
          "levels": K, "passes": passes,
          "ratio_masked_over_white": [round(p["render_masked"]["host_median_s"] / p["render_white"]["host_median_s"], 3) for p in passes]}

line = {"box": socket.gethostname(), "utterance_samples": N, "levels": K, "recordings": len(MASKERS), "recording_samples": len(MASKERS[0]),
        "snr_db": list(SNRS), "reps": args.reps, "warm": args.warm, "f2_masker_levels": levels, "cases": cases, "render": render}
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
ctx.close()
