#!/usr/bin/env python3
"""Rate of `cnn eval` with a hop (f2_eval_batch_strided) and without (f2_eval_batch), this tree's library against another build.

  eval_hop_rate.py build-baseline REV DIR      extract REV's library sources (git archive) into DIR and build them there
  eval_hop_rate.py ab BASELINE.so OUT.json [--rounds 2] [--batches 8,1000] [--hops 1,16,160] [--reps 3]
        alternates fresh processes, BASELINE.so and the tree's library: each runs f2_eval_batch and f2_eval_batch_strided at
        each hop on the same seeded batches of 1 s utterances in device memory; writes every run and a summary in which
        every entry point of the tree is held against the same entry point of the baseline
  eval_hop_rate.py measure every|strided|both OUT.json ...      one such process (F2CNN_PROBE_LIB picks the library)

Per case: one warm-up call, `reps` calls each between two device events (profiling off), then one call with f2_prof_enable
for the per-kernel device times. audio-s/s = audio seconds of the batch over the mean event time. The spread quoted for the
baseline is (max - min) / mean over all its timed calls of all rounds: the margin a difference has to exceed."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, RADIUS, STEP, N, FS = 128, 5, 160, 16000, 16000


def build_baseline(rev, dest):
    os.makedirs(dest, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "f2cnn_amd/build.py", "f2cnn_amd/csrc", "include"], check=True,
                         stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", dest], input=tar, check=True)
    subprocess.run([sys.executable, os.path.join(dest, "f2cnn_amd", "build.py")], check=True, stdout=subprocess.DEVNULL)
    print(os.path.join(dest, "f2cnn_amd", "lib", "libf2cnn_hip.so"))


def measure(which, out, batches, hops, reps):
    import numpy as np
    sys.path.insert(0, ROOT)
    if os.environ.get("F2CNN_PROBE_LIB"):
        from f2cnn_amd import build
        build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
    import bench
    from f2cnn_amd import _lib
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel
    ctx = _lib.Context(0)
    coefs = filters.make_erb_filters(FS, filters.centre_freqs(FS, C, 100))
    h = F2CNNModel.glorot(7).handle(ctx)
    nb = N - (2 * RADIUS + 1) * STEP
    cases = []
    for B in batches:
        waves = bench.synth_batch(bench.SEEDS["cfg4"], 0, B, N)
        offsets = np.arange(B + 1, dtype=np.int64) * N
        d_wave, d_scores, d_labels = ctx.malloc(waves.nbytes), ctx.malloc(8 * nb * B), ctx.malloc(nb * B)
        ctx.h2d(d_wave, waves)
        for entry, hop in [(e, h) for e in (("every", "strided") if which == "both" else (which,))
                           for h in (hops if e == "strided" else [1])]:
            if entry == "strided":
                windows = B * _lib.strided_window_count(N, RADIUS, STEP, hop)
                call = lambda: ctx.eval_batch_strided(h, d_wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS,
                                                      STEP, hop, d_scores, d_labels, _lib.MEM_DEVICE)
            else:
                windows = B * nb
                call = lambda: ctx.eval_batch(h, d_wave, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, RADIUS, STEP,
                                              d_scores, d_labels, _lib.MEM_DEVICE)
            call()
            ctx.synchronize()
            ms = []
            e0, e1 = ctx.event(), ctx.event()
            for _ in range(reps):
                ctx.record(e0)
                call()
                ctx.record(e1)
                ctx.synchronize()
                ms.append(ctx.elapsed_ms(e0, e1))
            for ev in (e0, e1):
                ctx.destroy_event(ev)
            ctx.prof_enable(True)
            call()
            kernels = {k: [n, round(t, 4)] for k, (n, t) in ctx.prof_get().items()}
            ctx.prof_enable(False)
            mean = sum(ms) / len(ms)
            case = {"entry": "f2_eval_batch_strided" if entry == "strided" else "f2_eval_batch", "batch": B, "hop": hop,
                    "windows": windows, "ms": [round(v, 4) for v in ms], "audio_s_per_s": round(B * N / FS / (mean / 1e3), 1),
                    "kernels_launches_ms": kernels}
            print(json.dumps(case), flush=True)
            cases.append(case)
        for p in (d_wave, d_scores, d_labels):
            ctx.free(p)
    ctx.close()
    json.dump(cases, open(out, "w"), indent=1)


def summarise(runs):
    def cases(lib, B, entry, hop):
        return [c for r in runs if r["lib"] == lib for c in r["cases"] if (c["batch"], c["entry"], c["hop"]) == (B, entry, hop)]

    def ns_per_window(c, kernel):       # device time of one profiling bracket per evaluated window
        return c["kernels_launches_ms"][kernel][1] * 1e6 / c["windows"]

    def side(cs, B):
        ms = [v for c in cs for v in c["ms"]]
        mean = sum(ms) / len(ms)
        win = [ns_per_window(c, "k_gather_windows") for c in cs]
        k = cs[-1]["kernels_launches_ms"]
        total = sum(v[1] for v in k.values())
        return {"windows": cs[-1]["windows"], "ms_mean": round(mean, 4), "ms_min": min(ms), "ms_max": max(ms),
                "spread": round((max(ms) - min(ms)) / mean, 4), "audio_s_per_s": round(B * N / FS / (mean / 1e3), 1),
                "window_stage_ns_per_window": [round(v, 3) for v in win], "window_stage_ns_per_window_mean": round(sum(win) / len(win), 3),
                "cnn_ns_per_window": [round(ns_per_window(c, "k_cnn_forward"), 2) for c in cs], "kernels_launches_ms": k,
                "share_of_kernel_time": {name: round(v[1] / total, 4) for name, v in k.items()}}
    out = {}
    keys = sorted({(c["batch"], c["entry"], c["hop"]) for r in runs for c in r["cases"]})
    for B, entry, hop in keys:
        old, new = cases("baseline", B, entry, hop), cases("tree", B, entry, hop)
        if not old or not new:
            continue
        o, n = side(old, B), side(new, B)
        # the tree's mean call time inside the baseline's own min .. max; its window stage within that relative spread
        verdict = {"ms_over_baseline": round(n["ms_mean"] / o["ms_mean"], 4),
                   "call_mean_within_baseline_min_max": bool(n["ms_mean"] <= o["ms_max"]),
                   "window_stage_over_baseline": round(n["window_stage_ns_per_window_mean"] / o["window_stage_ns_per_window_mean"], 4),
                   "window_stage_within_baseline_spread": bool(n["window_stage_ns_per_window_mean"] <=
                                                               o["window_stage_ns_per_window_mean"] * (1 + o["spread"]))}
        out.setdefault(f"{B} x 1 s", {})[entry + (f" hop {hop}" if entry.endswith("strided") else "")] = \
            {"baseline": o, "tree": n, "tree against baseline": verdict}
    return out


def ab(baseline, out, rounds, batches, hops, reps):
    tmp = os.path.join(os.path.dirname(os.path.abspath(out)), "eval_hop_rate_run.json")
    runs = []
    common = ["--batches", ",".join(map(str, batches)), "--hops", ",".join(map(str, hops)), "--reps", str(reps)]
    for rnd in range(rounds):
        for lib, path in (("baseline", baseline), ("tree", None)):
            env = dict(os.environ, F2CNN_PROBE_OLD_LIB="1")
            env.pop("F2CNN_PROBE_LIB", None)
            if path:
                env["F2CNN_PROBE_LIB"] = path
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "measure", "both", tmp] + common, env=env, timeout=900)
            if res.returncode != 0:      # nothing more is started on the device after a failed run
                sys.exit(f"{lib} run of round {rnd} ended with status {res.returncode}")
            runs.append({"lib": lib, "round": rnd, "cases": json.load(open(tmp))})
            os.remove(tmp)
    doc = {"method": __doc__.split("\n\n")[-1].replace("\n", " "), "shape": f"{C} channels, {N} samples per utterance, radius "
           f"{RADIUS}, step {STEP}, no low-pass, float32 FFT, device buffers", "summary": summarise(runs), "runs": runs}
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(doc["summary"], indent=1))


if __name__ == "__main__":
    ints = lambda s: [int(v) for v in s.split(",")]
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("build-baseline")
    p.add_argument("rev")
    p.add_argument("dest")
    for name in ("ab", "measure"):
        p = sub.add_parser(name)
        p.add_argument("first")          # ab: the baseline library; measure: every | strided | both
        p.add_argument("out")
        p.add_argument("--rounds", type=int, default=2)
        p.add_argument("--batches", type=ints, default=[8, 1000])
        p.add_argument("--hops", type=ints, default=[1, 16, 160])
        p.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.cmd == "build-baseline":
        build_baseline(a.rev, a.dest)
    elif a.cmd == "measure":
        measure(a.first, a.out, a.batches, a.hops, a.reps)
    else:
        ab(os.path.abspath(a.first), a.out, a.rounds, a.batches, a.hops, a.reps)
