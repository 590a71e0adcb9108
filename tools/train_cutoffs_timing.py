"""What rendering the training windows at an envelope cutoff per file costs (`cnn train --engine hip --from-wav --augment-cutoffs
...`), beside the render without cutoffs of the same build, beside that render of another build of the library, the pick kernel
alone, and the route the stage replaces. Warm context; host clock around work that ends in a device synchronise, HIP events around
the same work; median of --repeats; the builds alternated, two passes. Each build runs in a process of its own (a process holds one
library).

    (a) render           Trainer.render(): the tree's and --parent-lib's
    (b) render_filtered  Trainer.render(cutoffs=..., cutoff_of=...), a level per file drawn from the cutoffs or unfiltered (the
                         tree's build only)
    (c) pick             --kernel-utterances x --seconds of envelopes in device memory (a render's group), f2_lowpass_pick in place
                         by HIP events around the device call: every file at one cutoff, cutoff by cutoff, the drawn levels, and
                         every file unfiltered. Bytes: 16 per sample of a filtered file (read once, written once), as a share of the
                         8 TB/s HBM peak.
    (d) levels           the route there was: f2_lowpass_levels with K = 1 on the same envelopes, once per distinct cutoff (reads
                         the envelopes, writes the filtered block and the copy: 24 bytes per sample), in front of the plain gather;
                         the same call with the parent's build shows what the shared device function did to k_lowpass_levels

    python3 tools/train_cutoffs_timing.py [--parent-lib build/parent/libf2cnn_hip.so] [--utterances 400] [--seconds 3] [--centres 164]
                                          [--cutoffs 5,10,20,50] [--repeats 3] [--passes 2] [--out profiles/rNN.json]
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
PEAK_HBM = 8.0e12
CUTOFF_STREAM = 0x6375746F                      # Training.CUTOFF_STREAM (a parent build's Training.py does not have it)


def child(a):
    """One build's measurements, one JSON line on stdout"""
    lib = a.lib or os.environ.get("F2CNN_PROBE_LIB")
    if lib:
        from f2cnn_amd import build
        build.LIB_PATH = os.path.abspath(lib)
    from f2cnn_amd import _lib
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.scripts.CNN import Training
    from f2cnn_amd.trainer import Trainer
    tree = not a.lib
    seed, n = 3, int(a.seconds * FS)
    rng = np.random.default_rng(seed)
    reach = RADIUS * STEP
    waves = [(rng.standard_normal(n) * 3000).astype(np.int16) for _ in range(a.utterances)]
    centres = [np.linspace(reach, n - 1 - reach, a.centres).astype(np.int64) for _ in range(a.utterances)]
    signs = [rng.integers(0, 2, a.centres).astype(np.uint8) for _ in range(a.utterances)]
    freqs = filters.centre_freqs(FS, CHANNELS, 100)
    coefs = np.ascontiguousarray(filters.make_erb_filters(FS, freqs), dtype=np.float64)
    cutoffs = tuple(float(v) for v in a.cutoffs.split(",") if v)
    Kc = len(cutoffs)
    ctx = _lib.default_context()
    e0, e1 = ctx.event(), ctx.event()
    trainer = Trainer(F2CNNModel.glorot(seed, ROWS, CHANNELS), lr=1e-4, decay=1e-6, drop=Training.DROPOUT, seed=seed, ctx=ctx)
    trainer.set_waves(waves, centres, signs, coefs, RADIUS, STEP, group=Training.RENDER_GROUP)

    def timed(fn):
        """(host seconds, device ms) of fn, which ends in a device synchronise"""
        t0 = time.perf_counter()
        ctx.record(e0)
        fn()
        ctx.record(e1)
        dt = time.perf_counter() - t0
        ctx.synchronize()
        return dt, ctx.elapsed_ms(e0, e1)

    cases = {"render": lambda d: timed(trainer.render)}
    cut_rng = np.random.default_rng([seed, CUTOFF_STREAM])
    draws = [cut_rng.integers(0, Kc + 1, a.utterances).astype(np.int32) for _ in range(a.repeats + 1)]
    if tree:
        cases["render_filtered"] = lambda d: timed(lambda: trainer.render(cutoffs=cutoffs, cutoff_of=d))
    for fn in cases.values():
        fn(draws[0])                                                        # warm
    got = {k: [] for k in cases}
    for r in range(a.repeats):
        for k, fn in cases.items():                                         # alternating
            got[k].append(fn(draws[r + 1]))
    out = {k: {"host_s": [round(h, 5) for h, _ in v], "device_ms": [round(d, 3) for _, d in v],
               "host_median_s": statistics.median(h for h, _ in v), "device_median_ms": statistics.median(d for _, d in v)}
           for k, v in got.items()}
    if tree:
        out["render_filtered"]["filtered_share_of_files"] = [round(float((d < Kc).mean()), 4) for d in draws[1:]]
    trainer.close()

    # (c), (d): the filter calls alone on the envelopes of one group
    B = a.kernel_utterances
    flat = np.concatenate(waves[:B])
    offsets = np.arange(B + 1, dtype=np.int64) * n
    samples = CHANNELS * flat.size
    d_wave, d_env, d_lev = ctx.malloc(flat.nbytes), ctx.malloc(8 * samples), ctx.malloc(16 * samples)
    ctx.h2d(d_wave, flat)
    ctx.filterbank_envelope_fused(d_wave, _lib.WAVE_I16, offsets, coefs, B, CHANNELS, False, 0.0, _lib.FFT_F32, d_env, None, _lib.MEM_DEVICE)
    ctx.synchronize()

    def events(fn, reps):
        times = []
        for r in range(reps + 2):
            ctx.synchronize()
            ctx.record(e0)
            fn()
            ctx.record(e1)
            ctx.synchronize()
            if r >= 2:
                times.append(ctx.elapsed_ms(e0, e1))
        return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}

    stage = {"utterances": B, "envelope_bytes": 8 * samples, "reps": a.kernel_reps, "peak_hbm_bytes_per_s": PEAK_HBM, "levels_k1": {}}
    for c in cutoffs:
        t = events(lambda: ctx.lowpass_levels(d_env, offsets, B, CHANNELS, (c,), d_lev, _lib.MEM_DEVICE), a.kernel_reps)
        stage["levels_k1"]["{:g} Hz".format(c)] = {"ms": t, "fraction_of_hbm_peak": round(24 * samples / (t["median"] * 1e-3) / PEAK_HBM, 4)}
    stage["levels_k1_all_cutoffs_ms"] = round(sum(v["ms"]["median"] for v in stage["levels_k1"].values()), 4)
    if tree:
        stage["pick_in_place"] = {}
        drawn = np.random.default_rng([seed, 0x6B65726E]).integers(0, Kc + 1, B).astype(np.int32)
        named = [("{:g} Hz".format(c), np.full(B, l, np.int32)) for l, c in enumerate(cutoffs)]
        for name, cutoff_of in named + [("drawn", drawn), ("unfiltered", np.full(B, Kc, np.int32))]:
            # (in place over and over: a low-pass of gain <= 1 keeps the values finite)
            t = events(lambda: ctx.lowpass_pick(d_env, offsets, B, CHANNELS, cutoffs, cutoff_of, d_env, _lib.MEM_DEVICE), a.kernel_reps)
            share = float((cutoff_of < Kc).mean())
            stage["pick_in_place"][name] = {"ms": t, "filtered_share_of_files": round(share, 4), "bytes": int(16 * samples * share),
                                            "fraction_of_hbm_peak": round(16 * samples * share / (t["median"] * 1e-3) / PEAK_HBM, 4)}
    out["stage"] = stage
    for p in (d_wave, d_env, d_lev):
        ctx.free(p)
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
    ap.add_argument("--cutoffs", default="5,10,20,50")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--kernel-utterances", type=int, default=64)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        return child(a)
    passed = [arg for arg in (argv if argv is not None else sys.argv[1:])]
    builds = [("tree", None)] + ([("parent", a.parent_lib)] if a.parent_lib else [])
    result = {"workload": "{} utterances of {} s with {} centres each ({} windows of {}x{}), rendered {} at a time; a level per file drawn "
                          "from cutoffs {} Hz and unfiltered; the filter calls alone on {} x {} s".format(
                              a.utterances, a.seconds, a.centres, a.utterances * a.centres, ROWS, CHANNELS, 64, a.cutoffs,
                              a.kernel_utterances, a.seconds),
              "clock": "time.perf_counter around work that ends in a device synchronise and HIP events around the same work; the filter "
                       "calls by HIP events around the device call; median of {} after a warm round, cases alternated inside a process, "
                       "builds alternated, {} passes".format(a.repeats, a.passes),
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
