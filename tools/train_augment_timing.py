"""What re-rendering the training windows under fresh noise costs beside the epoch it feeds (`cnn train --engine hip --from-wav
--augment-snrs`): a trainer that owns the waves of a corpus (f2_trainer_set_waves), one epoch of f2_trainer_steps on the rendered
set, f2_trainer_render, and both together. Warm context, host clock around work that ends in a device synchronise, median of
--repeats, the three cases alternated inside a pass, two passes.

    (a) steps          one epoch on the rendered set
    (b) render+steps   what an augmented epoch costs
    (c) render         alone; HIP events around it give the device time, and the same events around f2_noise_pick (device memory) on
                       the same groups, levels and seed give the share of the two noise kernels - the rest is filterbank, envelope
                       and window gather

    python3 tools/train_augment_timing.py [--utterances 400] [--seconds 3] [--centres 164] [--batches 32,256] [--repeats 3]
                                          [--out profiles/r27_train_augment_timing.json]
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from f2cnn_amd import _lib                                   # noqa: E402
from f2cnn_amd.gammatone import filters                      # noqa: E402
from f2cnn_amd.model import F2CNNModel                      # noqa: E402
from f2cnn_amd.scripts.CNN import Training                   # noqa: E402
from f2cnn_amd.trainer import Trainer                        # noqa: E402

ROWS, CHANNELS, RADIUS, STEP, FS = 11, 128, 5, 160, 16000
SNRS = (20.0, 10.0, 5.0, 0.0)
GROUP = Training.RENDER_GROUP


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=400)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--centres", type=int, default=164)
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    seed, n = 3, int(a.seconds * FS)
    rng = np.random.default_rng(seed)
    reach = RADIUS * STEP
    waves = [(rng.standard_normal(n) * 3000).astype(np.int16) for _ in range(a.utterances)]
    centres = [np.linspace(reach, n - 1 - reach, a.centres).astype(np.int64) for _ in range(a.utterances)]
    signs = [rng.integers(0, 2, a.centres).astype(np.uint8) for _ in range(a.utterances)]
    windows = a.utterances * a.centres
    coefs = np.ascontiguousarray(filters.make_erb_filters(FS, filters.centre_freqs(FS, CHANNELS, 100)), dtype=np.float64)
    ctx = _lib.default_context()
    noise_rng = np.random.default_rng([seed, Training.NOISE_STREAM])

    # the noise kernels alone, on device copies of the groups' waves
    flat = np.concatenate(waves)
    offsets = np.arange(a.utterances + 1, dtype=np.int64) * n
    d_wave, d_noisy = ctx.malloc(flat.nbytes), ctx.malloc(8 * GROUP * n)
    ctx.h2d(d_wave, flat)
    ctx.synchronize()
    e0, e1 = ctx.event(), ctx.event()

    def noise_ms(level_of, noise_seed):
        ctx.record(e0)
        for g in range(0, a.utterances, GROUP):
            nb = min(GROUP, a.utterances - g)
            ctx.noise_pick(d_wave + 2 * int(offsets[g]), _lib.WAVE_I16, offsets[g:g + nb + 1] - offsets[g], nb, SNRS, level_of[g:g + nb], g,
                           noise_seed, d_noisy, _lib.MEM_DEVICE)
        ctx.record(e1)
        return ctx.elapsed_ms(e0, e1)

    result = {"workload": "{} utterances of {} s with {} centres each: {} windows of {}x{}, rendered {} utterances at a time at the levels "
                          "{} dB or clean".format(a.utterances, a.seconds, a.centres, windows, ROWS, CHANNELS, GROUP, list(SNRS)),
              "clock": "time.perf_counter around work that ends in a device synchronise; median of {} after a warm round, the cases "
                       "alternated, {} passes; render_device_ms / noise_device_ms: HIP events".format(a.repeats, a.passes),
              "box": socket.gethostname(), "audio_seconds": a.utterances * a.seconds, "batches": {}}
    for batch in [int(b) for b in a.batches.split(",")]:
        trainer = Trainer(F2CNNModel.glorot(seed, ROWS, CHANNELS), lr=1e-4, decay=1e-6, drop=Training.DROPOUT, seed=seed, ctx=ctx)
        trainer.set_waves(waves, centres, signs, coefs, RADIUS, STEP, group=GROUP)
        device_ms = {"render": [], "noise": []}

        def draw():
            return Training.draw_epoch_noise(noise_rng, len(SNRS), a.utterances)

        def steps():
            t0 = time.perf_counter()
            trainer.steps(rng.permutation(windows), batch)
            return time.perf_counter() - t0

        def render():
            level_of, noise_seed = draw()
            t0 = time.perf_counter()
            ctx.record(e0)
            trainer.render(SNRS, level_of, noise_seed)              # (returns after its one wait for the stream)
            ctx.record(e1)
            dt = time.perf_counter() - t0
            device_ms["render"].append(ctx.elapsed_ms(e0, e1))
            device_ms["noise"].append(noise_ms(level_of, noise_seed))
            return dt

        def render_steps():
            level_of, noise_seed = draw()
            t0 = time.perf_counter()
            trainer.render(SNRS, level_of, noise_seed)
            trainer.steps(rng.permutation(windows), batch)
            return time.perf_counter() - t0

        cases = {"steps": steps, "render_steps": render_steps, "render": render}
        for fn in (render, steps, render_steps):
            fn()                                                      # warm
        entry = {"passes": []}
        for _ in range(a.passes):
            for v in device_ms.values():
                v.clear()
            times = {k: [] for k in cases}
            for _ in range(a.repeats):
                for k, fn in cases.items():                           # alternating
                    times[k].append(fn())
            p = {k: {"seconds": v, "median_s": statistics.median(v)} for k, v in times.items()}
            p["render"]["render_device_ms"] = statistics.median(device_ms["render"])
            p["render"]["noise_device_ms"] = statistics.median(device_ms["noise"])
            p["render"]["rest_device_ms"] = p["render"]["render_device_ms"] - p["render"]["noise_device_ms"]
            p["render_over_steps"] = p["render"]["median_s"] / p["steps"]["median_s"]
            p["audio_seconds_per_s"] = a.utterances * a.seconds / p["render"]["median_s"]
            entry["passes"].append(p)
            print("batch {} pass {}: {}".format(batch, len(entry["passes"]), json.dumps(p)), flush=True)
        result["batches"][str(batch)] = entry
        trainer.close()
    ref = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r26_train_timing.json")
    if os.path.isfile(ref):
        with open(ref) as f:
            old = json.load(f)
        result["r26_train_timing_hip_epoch_s"] = {b: v["hip"]["median_s"] for b, v in old["batches"].items()}
        result["r26_note"] = "one epoch of 65536 random windows, profiles/r26_train_timing.json: measured earlier, on whichever box that run had"
    ctx.free(d_wave)
    ctx.free(d_noisy)
    ctx.destroy_event(e0)
    ctx.destroy_event(e1)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
