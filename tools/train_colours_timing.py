"""What rendering the training windows under coloured noise costs (`cnn train --engine hip --from-wav --augment-snrs ...
--augment-colours ...`), beside the white render of the same build at the same levels, beside the white render of another build of
the library, and the coloured stage alone. Warm context; host clock around work that ends in a device synchronise and HIP events;
median of --repeats; the builds alternated, two passes. Each build runs in a process of its own (a process holds one library).

    (a) render_white     Trainer.render(level SNRs, level_of, seed): the tree's and --parent-lib's
    (b) render_coloured  Trainer.render(..., firs=...) at the same level_of: a level is a (colour, SNR) pair, colour-major, the
                         filters noise.ColourFIR(colour, 16000, --taps) (the tree's build only)
    (c) stage            --kernel-utterances x --seconds in device memory, level_of drawn as in (a), HIP events around --inner
                         device calls: f2_shaped_noise_pick (sigma kernel + uploads + k_shaped_noise_pick) with the tile list
                         sorted by cost and in the natural order, each twice, and f2_noise_pick (sigma kernel + uploads +
                         k_noise_pick) on the same work. The difference of the two calls is what the filtering costs; the FMAs
                         are n * T_level per utterance, given as FMAs per second of that difference and of the whole call, and
                         as a share of the 39.3 T FMA/s float64 vector peak.

    python3 tools/train_colours_timing.py [--parent-lib build/parent/libf2cnn_hip.so] [--utterances 400] [--seconds 3] [--centres 164]
                                          [--colours white,pink,speech] [--snrs 20,10] [--taps 1025] [--repeats 3] [--passes 2]
                                          [--out profiles/rNN.json]
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ROWS, CHANNELS, RADIUS, STEP, FS = 11, 128, 5, 160, 16000
PEAK_FMA = 39.3e12


def child(a):
    """One build's measurements, one JSON line on stdout"""
    lib = a.lib or os.environ.get("F2CNN_PROBE_LIB")
    if lib:
        from f2cnn_amd import build
        build.LIB_PATH = os.path.abspath(lib)
    from f2cnn_amd import _lib, noise
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Training
    from f2cnn_amd.scripts.CNN.Evaluating import ColourLevels
    from f2cnn_amd.trainer import Trainer
    tree = not a.lib
    seed, n = 3, int(a.seconds * FS)
    rng = np.random.default_rng(seed)
    reach = RADIUS * STEP
    waves = [(rng.standard_normal(n) * 3000).astype(np.int16) for _ in range(a.utterances)]
    centres = [np.linspace(reach, n - 1 - reach, a.centres).astype(np.int64) for _ in range(a.utterances)]
    signs = [rng.integers(0, 2, a.centres).astype(np.uint8) for _ in range(a.utterances)]
    coefs = np.ascontiguousarray(filters.make_erb_filters(FS, filters.centre_freqs(FS, CHANNELS, 100)), dtype=np.float64)
    grid = ColourLevels(a.colours.split(","), [float(v) for v in a.snrs.split(",")])
    firs = [noise.FromSpec(spec, FS, a.taps) for spec, _, _ in grid]
    snrs = [v for _, _, v in grid]
    K = len(grid)
    ctx = _lib.default_context()
    e0, e1 = ctx.event(), ctx.event()
    trainer = Trainer(F2CNNModel.glorot(seed, ROWS, CHANNELS), lr=1e-4, decay=1e-6, drop=Training.DROPOUT, seed=seed, ctx=ctx)
    trainer.set_waves(waves, centres, signs, coefs, RADIUS, STEP, group=Training.RENDER_GROUP)
    noise_rng = np.random.default_rng([seed, Training.NOISE_STREAM])
    draws = [Training.draw_epoch_noise(noise_rng, K, a.utterances) for _ in range(a.repeats + 1)]       # the same for every case

    def timed(fn):
        """(host seconds, device ms) of fn, which ends in a device synchronise"""
        t0 = time.perf_counter()
        ctx.record(e0)
        fn()
        ctx.record(e1)
        dt = time.perf_counter() - t0
        ctx.synchronize()
        return dt, ctx.elapsed_ms(e0, e1)

    cases = {"render_white": lambda d: timed(lambda: trainer.render(snrs, d[0], d[1]))}
    if tree:
        cases["render_coloured"] = lambda d: timed(lambda: trainer.render(snrs, d[0], d[1], firs=firs))
    for fn in cases.values():
        fn(draws[0])                                                        # warm
    got = {k: [] for k in cases}
    for r in range(a.repeats):
        for k, fn in cases.items():                                         # alternating
            got[k].append(fn(draws[r + 1]))
    out = {k: {"host_s": [round(h, 5) for h, _ in v], "device_ms": [round(d, 3) for _, d in v],
               "host_median_s": statistics.median(h for h, _ in v), "device_median_ms": statistics.median(d for _, d in v)}
           for k, v in got.items()}
    trainer.close()

    # (c) the stage alone
    B = a.kernel_utterances
    level_of = np.random.default_rng([seed, 0x6B65726E]).integers(0, K + 1, B).astype(np.int32)
    flat = np.concatenate(waves[:B])
    offsets = np.arange(B + 1, dtype=np.int64) * n
    d_wave, d_out = ctx.malloc(flat.nbytes), ctx.malloc(8 * flat.size)
    ctx.h2d(d_wave, flat)
    ctx.synchronize()
    work = sum(n * len(firs[l]) for l in level_of if l < K)

    def events(fn):
        for _ in range(3):
            fn()
        ctx.synchronize()
        times, enqueue = [], []
        for _ in range(a.kernel_reps):
            ctx.record(e0)
            t0 = time.perf_counter()
            for _ in range(a.inner):
                fn()
            enqueue.append((time.perf_counter() - t0) * 1e3 / a.inner)      # what the host takes to enqueue a call: where this is
            ctx.record(e1)                                                  # not below the event time, the events time the host
            ctx.synchronize()
            times.append(ctx.elapsed_ms(e0, e1) / a.inner)
        return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4),
                "host_enqueue_median": round(statistics.median(enqueue), 4)}

    def white():
        ctx.noise_pick(d_wave, _lib.WAVE_I16, offsets, B, snrs, level_of, 0, seed, d_out, _lib.MEM_DEVICE)

    def coloured():
        ctx.shaped_noise_pick(d_wave, _lib.WAVE_I16, offsets, B, snrs, firs, level_of, 0, seed, d_out, _lib.MEM_DEVICE)

    stage = {"utterances": B, "levels_drawn": [int((level_of == l).sum()) for l in range(K + 1)], "taps": [len(h) for h in firs],
             "useful_fmas": work, "calls_per_measurement": a.inner, "reps": a.kernel_reps, "peak_fma_per_s": PEAK_FMA,
             "noise_pick_call_ms": events(white)}
    if tree:
        # (the two orders twice, the second time the other way round: neither owns the warmer part of the run)
        for name, sort in (("sorted", 1), ("natural", 0), ("natural_again", 0), ("sorted_again", 1)):
            with ctx.options(noise_pick_sort=sort):
                call = events(coloured)
            extra = max(call["median"] - stage["noise_pick_call_ms"]["median"], 1e-6)
            stage["shaped_noise_pick_" + name] = {
                "call_ms": call, "tfma_per_s_of_call": round(work / (call["median"] * 1e-3) / 1e12, 3),
                "ms_beyond_noise_pick": round(extra, 4), "tfma_per_s_beyond_noise_pick": round(work / (extra * 1e-3) / 1e12, 3),
                "fraction_of_float64_vector_peak_beyond_noise_pick": round(work / (extra * 1e-3) / PEAK_FMA, 4)}
    out["stage"] = stage
    ctx.free(d_wave)
    ctx.free(d_out)
    ctx.destroy_event(e0)
    ctx.destroy_event(e1)
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="another build of the library (the parent commit's) to measure beside the tree's")
    ap.add_argument("--utterances", type=int, default=400)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--centres", type=int, default=164)
    ap.add_argument("--colours", default="white,pink,speech")
    ap.add_argument("--snrs", default="20,10")
    ap.add_argument("--taps", type=int, default=1025)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--kernel-utterances", type=int, default=64)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        return child(a)
    passed = [arg for arg in (argv if argv is not None else sys.argv[1:])]
    builds = [("tree", None)] + ([("parent", a.parent_lib)] if a.parent_lib else [])
    result = {"workload": "{} utterances of {} s with {} centres each ({} windows of {}x{}), rendered {} at a time; a level per file drawn "
                          "from colours {} x SNRs {} dB ({} taps) and clean; stage on {} x {} s".format(
                              a.utterances, a.seconds, a.centres, a.utterances * a.centres, ROWS, CHANNELS, 64, a.colours, a.snrs, a.taps,
                              a.kernel_utterances, a.seconds),
              "clock": "time.perf_counter around work that ends in a device synchronise and HIP events around the same work; median of {} "
                       "after a warm round, cases alternated inside a process, builds alternated, {} passes".format(a.repeats, a.passes),
              "box": socket.gethostname(), "passes": []}
    for _ in range(a.passes):
        entry = {}
        for name, lib in builds:                                            # alternating, each in a fresh process
            env = dict(os.environ)
            cmd = [sys.executable, os.path.abspath(__file__), "--child"] + passed
            if lib:
                cmd += ["--lib", lib]
                env["F2CNN_PROBE_OLD_LIB"] = "1"                            # (a build without the new symbols still loads)
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=600)
            lines = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not lines:
                print(res.stdout)
                raise RuntimeError("the {} build's measurements ended with status {}".format(name, res.returncode))
            entry[name] = json.loads(lines[-1][len("RESULT "):])
            print("pass {} {}: {}".format(len(result["passes"]) + 1, name, json.dumps(entry[name])), flush=True)
        result["passes"].append(entry)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
