"""The fused figure / occlusion / saliency calls of two builds of the library (profiles/r37_a_figure_timing_old_new.json), by the
method of tools/train_timing_old_new.py:
tools/eval_figure_timing.py, tools/occlusion_timing.py and tools/saliency_timing.py --no-torch, each in a process of its own per
build (F2CNN_PROBE_LIB), the builds alternating old, new, old, new. Per figure: min of the mins, median of the medians, max of
the maxes over the rounds; the bar: new median <= old median + old max - old min.
    python3 tools/figure_timing_old_new.py OLD_LIB NEW_LIB OUT.json [--rounds 2]"""
import argparse, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = [   # name of the fused call's figures, command
    ("eval_figure_batch", ["tools/eval_figure_timing.py", "--reps", "3", "--warm", "1"]),
    ("eval_occlusion_batch", ["tools/occlusion_timing.py", "--reps", "3", "--warm", "1"]),
    ("eval_saliency_batch", ["tools/saliency_timing.py", "--no-torch", "--reps", "3", "--warm", "1"]),
]


def child(cmd, lib):
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable] + cmd, env=dict(os.environ, F2CNN_PROBE_LIB=lib), stdout=subprocess.PIPE, text=True, timeout=400, cwd=ROOT)
    if out.returncode != 0:
        print(f"{' '.join(cmd)} -> exit status {out.returncode}; stopping", flush=True)
        sys.exit(2)
    print(f"  {cmd[0]}: {time.perf_counter() - t0:.0f} s", flush=True)
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_lib")
    ap.add_argument("new_lib")
    ap.add_argument("out")
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    libs = {"old": os.path.abspath(a.old_lib), "new": os.path.abspath(a.new_lib)}
    seen = {k: {} for k in libs}
    for r in range(a.rounds):
        for k, lib in libs.items():
            for name, cmd in TOOLS:
                res = child(cmd, lib)
                for c in res["cases"]:
                    for mem in ("host", "resident"):
                        for clock in ("event", "wall"):
                            u = c.get("utterances", res.get("utterances"))
                            seen[k].setdefault(f"f2_{name}, {u} utterances, hop {c['hop']}, {mem}: {clock} ms", []).append(c[mem][f"{name}_{clock}_ms"])
            print(f"round {r + 1} {k} done", flush=True)
    result = {"method": __doc__, "rounds": a.rounds, "figures": {}}
    bad = 0
    for name in seen["old"]:
        f = {k: {"min": min(p["min"] for p in seen[k][name]), "median": statistics.median(p["median"] for p in seen[k][name]),
                 "max": max(p["max"] for p in seen[k][name]), "n": 6 * len(seen[k][name])} for k in libs}
        f["bar"] = round(f["old"]["median"] + f["old"]["max"] - f["old"]["min"], 3)
        f["within_bar"] = f["new"]["median"] <= f["bar"]
        bad += not f["within_bar"]
        result["figures"][name] = f
        print(f"{name}: old {f['old']['min']:.4g} / {f['old']['median']:.4g} / {f['old']['max']:.4g}, new {f['new']['min']:.4g} / "
              f"{f['new']['median']:.4g} / {f['new']['max']:.4g}, bar {f['bar']:.4g}: {'within' if f['within_bar'] else 'MISSED'}", flush=True)
    with open(a.out, "w") as fo:
        json.dump(result, fo, indent=1)
        fo.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
