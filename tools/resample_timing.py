"""256 utterances of 3 s at 44.1 kHz, stereo int16, to mono float64 at 16 kHz:
(a) f2_resample_batch on frames resident in device memory, output to device memory - HIP-event time per call over REPS
repeated calls after WARM unmeasured ones, and the bytes it has to read and write against the HBM peak - and
(b) scipy.signal.resample_poly on the mean of the channels in a pool of 16 processes, wall time of the whole batch (the
pool started and its workers warmed before the clock).
The device result is held against resample_poly on the first utterances before anything is timed.
Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, json, multiprocessing, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for cfg1_latency.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])

ap = argparse.ArgumentParser()
ap.add_argument("--utterances", type=int, default=256)
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--rate", type=int, default=44100)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--processes", type=int, default=16)
ap.add_argument("--out")
args = ap.parse_args()

TARGET, HBM_PEAK = 16000, 8e12


def host_one(stereo):
    from scipy.signal import resample_poly
    mono = (stereo[:, 0].astype(np.float64) + stereo[:, 1].astype(np.float64)) / 2
    return resample_poly(mono, TARGET, args.rate)


def stat(t):
    return {"mean": round(statistics.fmean(t), 4), "stdev": round(statistics.stdev(t), 4), "median": round(statistics.median(t), 4),
            "min": round(min(t), 4), "max": round(max(t), 4)}


if __name__ == "__main__":
    from f2cnn_amd import _lib, resample
    B, n = args.utterances, int(round(args.seconds * args.rate))
    rng = np.random.default_rng(17)
    audio = np.clip(np.round(rng.standard_normal((B * n, 2)) * 3000.0), -32768, 32767).astype(np.int16)
    offsets = np.arange(B + 1, dtype=np.int64) * n
    up, down, half_len, taps = resample.design_resampler(args.rate, TARGET)
    n_out = _lib.resampled_length(n, up, down)

    ctx = _lib.Context(0)
    d_audio, d_out = ctx.malloc(audio.nbytes), ctx.malloc(8 * B * n_out)
    ctx.h2d(d_audio, audio)
    call = lambda: ctx.resample_batch(d_audio, _lib.PCM_I16, 2, -1, offsets, B, up, down, taps, half_len, d_out, _lib.MEM_DEVICE)
    call()
    got = np.empty(B * n_out)
    ctx.d2h(got, d_out)
    worst = max(float(np.abs(got[b * n_out:(b + 1) * n_out] - host_one(audio[b * n:(b + 1) * n])).max()) for b in range(4))
    assert worst < 1e-8, worst
    e0, e1 = ctx.event(), ctx.event()
    device_ms = []
    for rep in range(args.warm + args.reps):
        ctx.record(e0)
        call()
        ctx.record(e1)
        if rep >= args.warm:
            device_ms.append(ctx.elapsed_ms(e0, e1))
    for p in (d_audio, d_out):
        ctx.free(p)
    ctx.close()

    pieces = [audio[b * n:(b + 1) * n] for b in range(B)]
    host_ms = []
    with multiprocessing.get_context("spawn").Pool(args.processes) as pool:
        pool.map(host_one, pieces[:2 * args.processes])          # workers started, scipy imported
        for _ in range(3):
            t0 = time.perf_counter()
            pool.map(host_one, pieces)
            host_ms.append((time.perf_counter() - t0) * 1e3)

    d, h = stat(device_ms), stat(host_ms)
    audio_s = B * n / args.rate
    moved = int(audio.nbytes + 8 * B * n_out)
    line = {"utterances": B, "frames": n, "rate_in": args.rate, "rate_out": TARGET, "channels": 2, "pcm": "int16", "up": up, "down": down,
            "taps": int(2 * half_len + 1), "taps_per_phase": int(-(-(2 * half_len + 1) // up)), "samples_out": int(B * n_out),
            "max_abs_difference_from_resample_poly": worst,
            "f2_resample_batch_device_event_ms": d, "reps": args.reps, "warm": args.warm,
            "bytes_read_plus_written": moved, "device_bytes_per_s": round(moved / (d["mean"] * 1e-3)),
            "fraction_of_hbm_peak": round(moved / (d["mean"] * 1e-3) / HBM_PEAK, 4), "hbm_peak_bytes_per_s": HBM_PEAK,
            "resample_poly_pool_wall_ms": h, "pool_processes": args.processes, "pool_passes": len(host_ms),
            "audio_s_per_s": {"f2_resample_batch_device": round(audio_s / d["mean"] * 1e3, 1),
                              "resample_poly_pool": round(audio_s / h["mean"] * 1e3, 1)},
            "host_ms_per_audio_second_per_core": round(h["mean"] * args.processes / audio_s, 3)}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
