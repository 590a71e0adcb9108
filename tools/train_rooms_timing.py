"""What rendering the training windows in a room per file costs (`cnn train --engine hip --from-wav --augment-t60`), beside the plain
render of another build of the library and beside the epoch it feeds, and k_reverb_pick alone against k_reverb_levels of that
other build on the same work. Warm context; host clock around work that ends in a device synchronise and HIP events; median of
--repeats; the builds alternated, two passes. Each build runs in a process of its own (a process holds one library).

    (a) render          Trainer.render(), no rooms: the tree's and --parent-lib's
    (b) render_wet      Trainer.render_wet with a room per file drawn from --t60 and dry (the tree's build only)
    (c) steps           one epoch of f2_trainer_steps at every batch size of --batches
    (d) kernels         --kernel-utterances x --seconds in device memory, rooms drawn as in (b), HIP events around --inner calls:
                        f2_reverb_pick with the tile list sorted by cost and in the natural order (the tree's build), and
                        f2_reverb_levels with ONE response at a time on the utterances that drew it, summed over the responses
                        (both builds: the same useful FMAs, sum_k min(k + 1, T) per utterance), as FMAs per second and as a share
                        of the 39.3 T FMA/s float64 vector peak

    python3 tools/train_rooms_timing.py [--parent-lib build/parent/libf2cnn_hip.so] [--utterances 400] [--seconds 3] [--centres 164]
                                        [--t60 0.2,0.4,0.8] [--batches 32,256] [--repeats 3] [--passes 2] [--out profiles/rNN.json]
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


def fmas(n, taps):
    """terms of sum_{t <= min(k, T - 1)} over k < n"""
    m = min(n, taps)
    return m * (m + 1) // 2 + (n - m) * taps


def child(a):
    """One build's measurements, one JSON line on stdout"""
    lib = a.lib or os.environ.get("F2CNN_PROBE_LIB")   # (the latter: another build measured as the tree is, render_wet and the pick kernel too)
    if lib:
        from f2cnn_amd import build
        build.LIB_PATH = os.path.abspath(lib)
    from f2cnn_amd import _lib
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.reverb import SyntheticRIR
    from f2cnn_amd.scripts.CNN import Training
    from f2cnn_amd.trainer import Trainer
    tree = not a.lib
    seed, n = 3, int(a.seconds * FS)
    rng = np.random.default_rng(seed)
    reach = RADIUS * STEP
    waves = [(rng.standard_normal(n) * 3000).astype(np.int16) for _ in range(a.utterances)]
    centres = [np.linspace(reach, n - 1 - reach, a.centres).astype(np.int64) for _ in range(a.utterances)]
    signs = [rng.integers(0, 2, a.centres).astype(np.uint8) for _ in range(a.utterances)]
    windows = a.utterances * a.centres
    coefs = np.ascontiguousarray(filters.make_erb_filters(FS, filters.centre_freqs(FS, CHANNELS, 100)), dtype=np.float64)
    t60 = [float(v) for v in a.t60.split(",")]
    Kr = len(t60)
    ctx = _lib.default_context()
    e0, e1 = ctx.event(), ctx.event()
    room_rng = np.random.default_rng([seed, Training.ROOM_STREAM]) if tree else None
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

    def render_wet():
        room_of, room_seed = Training.draw_epoch_rooms(room_rng, Kr, a.utterances)
        rirs = Training.build_rooms(t60, (), FS, 0.0, room_seed)           # (on the host, outside the clock: as an epoch would pay it,
        return timed(lambda: trainer.render_wet(rirs, room_of))            #  it is reported apart below)

    # (both builds walk the same cases in the same order, so that a render follows the same work in both)
    cases = {"render": lambda: timed(trainer.render)}
    if tree:
        cases["render_wet"] = render_wet
    for batch in [int(b) for b in a.batches.split(",")]:
        cases["steps_b{}".format(batch)] = lambda batch=batch: timed(lambda: trainer.steps(rng.permutation(windows), batch))
    for fn in cases.values():
        fn()                                                                # warm
    got = {k: [] for k in cases}
    for _ in range(a.repeats):
        for k, fn in cases.items():                                         # alternating
            got[k].append(fn())
    out = {k: {"host_s": [round(h, 5) for h, _ in v], "device_ms": [round(d, 3) for _, d in v],
               "host_median_s": statistics.median(h for h, _ in v), "device_median_ms": statistics.median(d for _, d in v)}
           for k, v in got.items()}
    if tree:
        t0 = time.perf_counter()
        Training.build_rooms(t60, (), FS, 0.0, 1)
        out["build_rooms_host_s"] = time.perf_counter() - t0
    trainer.close()

    # (d) the kernels alone
    B = a.kernel_utterances
    krng = np.random.default_rng([seed, 0x6B65726E])
    room_of = krng.integers(0, Kr + 1, B).astype(np.int32)
    rirs = [SyntheticRIR(v, FS, 0.0, 7, level) for level, v in enumerate(t60)]
    flat = np.concatenate(waves[:B])
    offsets = np.arange(B + 1, dtype=np.int64) * n
    order = np.argsort(room_of, kind="stable")                              # the utterances of a room side by side, for the sweep kernel
    by_room = np.concatenate([waves[b] for b in order])
    counts = [int((room_of == l).sum()) for l in range(Kr + 1)]
    first = np.concatenate([[0], np.cumsum(counts)])
    d_wave, d_sorted, d_out = ctx.malloc(flat.nbytes), ctx.malloc(flat.nbytes), ctx.malloc(8 * 2 * flat.size)
    ctx.h2d(d_wave, flat)
    ctx.h2d(d_sorted, by_room)
    ctx.synchronize()
    work = sum(fmas(n, len(rirs[l])) for l in room_of if l < Kr)

    def events(fn):
        for _ in range(3):
            fn()
        ctx.synchronize()
        times = []
        for _ in range(a.kernel_reps):
            ctx.record(e0)
            for _ in range(a.inner):
                fn()
            ctx.record(e1)
            ctx.synchronize()
            times.append(ctx.elapsed_ms(e0, e1) / a.inner)
        med = statistics.median(times)
        return {"call_ms": {"median": round(med, 4), "min": round(min(times), 4), "max": round(max(times), 4)},
                "tfma_per_s": round(work / (med * 1e-3) / 1e12, 3), "fraction_of_float64_vector_peak": round(work / (med * 1e-3) / PEAK_FMA, 4)}

    def levels_one_response_at_a_time():
        for l in range(Kr):
            if counts[l]:
                ctx.reverb_levels(d_sorted + 2 * int(first[l]) * n, _lib.WAVE_I16, offsets[:counts[l] + 1], counts[l], [rirs[l]], d_out,
                                  _lib.MEM_DEVICE)

    kernels = {"utterances": B, "rooms_drawn": counts, "taps": [len(h) for h in rirs], "useful_fmas": work, "calls_per_measurement": a.inner,
               "reps": a.kernel_reps, "peak_fma_per_s": PEAK_FMA, "reverb_levels_one_response_at_a_time": events(levels_one_response_at_a_time)}
    if tree:
        for name, sort in (("reverb_pick_sorted", 1), ("reverb_pick_natural", 0)):
            with ctx.options(reverb_pick_sort=sort):
                kernels[name] = events(lambda: ctx.reverb_pick(d_wave, _lib.WAVE_I16, offsets, B, rirs, room_of, d_out, _lib.MEM_DEVICE))
        # a second look at the two orders, the other way round: neither owns the warmer part of the run
        for name, sort in (("reverb_pick_natural_again", 0), ("reverb_pick_sorted_again", 1)):
            with ctx.options(reverb_pick_sort=sort):
                kernels[name] = events(lambda: ctx.reverb_pick(d_wave, _lib.WAVE_I16, offsets, B, rirs, room_of, d_out, _lib.MEM_DEVICE))
    out["kernels"] = kernels
    for p in (d_wave, d_sorted, d_out):
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
    ap.add_argument("--t60", default="0.2,0.4,0.8")
    ap.add_argument("--batches", default="32,256")
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
    result = {"workload": "{} utterances of {} s with {} centres each ({} windows of {}x{}), rendered {} at a time; rooms drawn per file from "
                          "t60 {} s and dry; kernels on {} x {} s".format(a.utterances, a.seconds, a.centres, a.utterances * a.centres, ROWS,
                                                                        CHANNELS, 64, a.t60, a.kernel_utterances, a.seconds),
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
