"""What rendering the training windows at a spectral resolution per file costs (`cnn train --engine hip --from-wav
--augment-spreads ... --augment-bands ...`), beside the render without matrices of the same build, beside that render of another
build of the library, the mixing gather alone beside the plain gather, and the route the mixing gather replaces. Warm context; host
clock around work that ends in a device synchronise, HIP events around the same work, and the library's own event pair around the
gather launch (f2_prof_*); median of --repeats; the builds alternated, two passes. Each build runs in a process of its own (a
process holds one library).

    (a) render          Trainer.render(): the tree's and --parent-lib's
    (b) render_smeared  Trainer.render(mixes=..., mix_of=...), a level per file drawn from the spreads, then the bands, or sharp
                        (the tree's build only)
    (c) gather          --kernel-utterances x --seconds of envelopes in device memory (a render's group), --centres windows each:
                        k_gather_windows<true> (no matrices) and k_gather_windows_mixed with every file at one level, level by level,
                        and with the drawn levels, by the event pair around the launch. FMAs: rows x the span a channel's tile walks,
                        summed over the channels (walked), and rows x the row's own support (useful), per window; as a share of the
                        39.3 T FMA/s float64 vector peak. Bytes: the window's float64 values read and float32 values written, as a
                        share of the 8 TB/s HBM peak.
    (d) whole envelopes the route the kernel replaces: f2_channel_mix_levels with K = 1 on the same envelopes (HIP events around the
                        device call), then the plain gather on the mixed block

    python3 tools/train_smear_timing.py [--parent-lib build/parent/libf2cnn_hip.so] [--utterances 400] [--seconds 3] [--centres 164]
                                        [--spreads 0.5,1,2,4] [--bands 16,8] [--repeats 3] [--passes 2] [--out profiles/rNN.json]
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
PEAK_FMA, PEAK_HBM = 39.3e12, 8.0e12
TILE = 16                                       # F2_SMEAR_TILE_CHANNELS: the rows whose supports one span unites


def fmas_per_window(W):
    """(walked, useful) FMAs of one window under the matrix W"""
    lo = np.array([np.flatnonzero(r)[0] if r.any() else 0 for r in W])
    hi = np.array([np.flatnonzero(r)[-1] + 1 if r.any() else 0 for r in W])
    walked = 0
    for c0 in range(0, len(W), TILE):
        live = hi[c0:c0 + TILE] > lo[c0:c0 + TILE]
        if live.any():
            walked += (hi[c0:c0 + TILE][live].max() - lo[c0:c0 + TILE][live].min()) * min(TILE, len(W) - c0)
    return int(ROWS * walked), int(ROWS * (hi - lo).sum())


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
    spreads = [float(v) for v in a.spreads.split(",") if v]
    bands = [int(v) for v in a.bands.split(",") if v]
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
    if tree:
        mixes, names = Training.build_smear_levels(spreads, bands, freqs)
        Km = len(names)
        smear_rng = np.random.default_rng([seed, Training.SMEAR_STREAM])
        draws = [Training.draw_epoch_smear(smear_rng, Km, a.utterances) for _ in range(a.repeats + 1)]
        cases["render_smeared"] = lambda d: timed(lambda: trainer.render(mixes=mixes, mix_of=d))
    else:
        draws = [None] * (a.repeats + 1)
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

    if tree:
        # (c), (d): the gathers alone on the envelopes of one group
        B = a.kernel_utterances
        flat = np.concatenate(waves[:B])
        offsets = np.arange(B + 1, dtype=np.int64) * n
        coff = np.arange(B + 1, dtype=np.int64) * a.centres
        cen = np.concatenate(centres[:B])
        nwin = int(coff[-1])
        env_bytes = 8 * CHANNELS * flat.size
        d_wave, d_env, d_win = ctx.malloc(flat.nbytes), ctx.malloc(env_bytes), ctx.malloc(4 * nwin * ROWS * CHANNELS)
        d_lev = ctx.malloc(2 * env_bytes)
        ctx.h2d(d_wave, flat)
        ctx.filterbank_envelope_fused(d_wave, _lib.WAVE_I16, offsets, coefs, B, CHANNELS, False, 0.0, _lib.FFT_F32, d_env, None, _lib.MEM_DEVICE)
        ctx.synchronize()

        def gather(env, mx, mix_of):
            """median kernel ms of the gather launch, by the library's event pair around it"""
            ms = []
            for r in range(a.kernel_reps + 2):
                ctx.prof_reset()
                ctx.gather_windows_mixed(env, offsets, B, CHANNELS, coff, cen, RADIUS, STEP, True, mx, mix_of, d_win, _lib.MEM_DEVICE)
                launches, total = ctx.prof_get()["k_gather_windows"]
                assert launches == 1
                if r >= 2:
                    ms.append(total)
            return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}

        ctx.prof_enable(True)
        window_bytes = ROWS * CHANNELS * 12
        plain = gather(d_env, None, None)
        stage = {"utterances": B, "windows": nwin, "reps": a.kernel_reps, "peak_fma_per_s": PEAK_FMA, "peak_hbm_bytes_per_s": PEAK_HBM,
                 "window_bytes": window_bytes, "plain_gather_ms": plain,
                 "plain_gather_fraction_of_hbm_peak": round(nwin * window_bytes / (plain["median"] * 1e-3) / PEAK_HBM, 4), "levels": {}}
        drawn = np.random.default_rng([seed, 0x6B65726E]).integers(0, Km + 1, B).astype(np.int32)
        for name, mix_of in [(nm, np.full(B, l, np.int32)) for l, nm in enumerate(names)] + [("drawn", drawn)]:
            t = gather(d_env, mixes, mix_of)
            per = [fmas_per_window(mixes[l]) if l < Km else (0, 0) for l in mix_of]
            walked, useful = (sum(p[i] for p in per) * a.centres for i in (0, 1))
            stage["levels"][name] = {
                "mixed_gather_ms": t, "times_the_plain_gather": round(t["median"] / plain["median"], 2), "walked_fmas": walked,
                "useful_fmas": useful, "walked_tfma_per_s": round(walked / (t["median"] * 1e-3) / 1e12, 3),
                "fraction_of_float64_vector_peak": round(walked / (t["median"] * 1e-3) / PEAK_FMA, 4),
                "fraction_of_hbm_peak": round(nwin * window_bytes / (t["median"] * 1e-3) / PEAK_HBM, 4)}
        ctx.prof_enable(False)

        # (d) one matrix over the whole envelopes, then the plain gather on that block
        def whole(level):
            times = []
            for r in range(a.kernel_reps // 4 + 2):
                ctx.synchronize()
                ctx.record(e0)
                ctx.channel_mix_levels(d_env, offsets, B, CHANNELS, mixes[level:level + 1], d_lev, _lib.MEM_DEVICE)
                ctx.record(e1)
                ctx.synchronize()
                if r >= 1:
                    times.append(ctx.elapsed_ms(e0, e1))
            return {"median": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}

        stage["whole_envelopes"] = {}
        for l, nm in enumerate(names):
            mix_ms = whole(l)
            ctx.prof_enable(True)
            g = gather(d_lev, None, None)
            ctx.prof_enable(False)
            total = mix_ms["median"] + g["median"]
            stage["whole_envelopes"][nm] = {"channel_mix_levels_ms": mix_ms, "plain_gather_ms": g, "total_ms": round(total, 4),
                                            "times_the_mixed_gather": round(total / stage["levels"][nm]["mixed_gather_ms"]["median"], 2)}
        out["stage"] = stage
        for p in (d_wave, d_env, d_win, d_lev):
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
    ap.add_argument("--spreads", default="0.5,1,2,4")
    ap.add_argument("--bands", default="16,8")
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
                          "from spreads {} ERB, bands {} and sharp; gathers alone on {} x {} s".format(
                              a.utterances, a.seconds, a.centres, a.utterances * a.centres, ROWS, CHANNELS, 64, a.spreads, a.bands,
                              a.kernel_utterances, a.seconds),
              "clock": "time.perf_counter around work that ends in a device synchronise and HIP events around the same work; the gathers by "
                       "the library's event pair around their launch; median of {} after a warm round, cases alternated inside a process, "
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
