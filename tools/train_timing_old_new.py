"""Host time per launch of two builds of the library where steps are shortest (profiles/r28_a_train_timing_old_new.json):
tools/train_timing.py --only-hip (one epoch of 65536 windows, batches 32 and 256) and tools/saliency_timing.py --no-torch
(f2_eval_saliency_batch, 1 and 16 utterances, hop 160 and 16), each in a process of its own per build (the library selected the
way tools/bench_with_lib.py does it), the two builds alternating: old, new, old, new, ...

    python3 tools/train_timing_old_new.py OLD_LIB NEW_LIB OUT.json [--rounds 3]

Per round and build: train_timing with a warm epoch and 2 measured ones, saliency_timing with 1 warm and 2 x 3 measured calls.
Train: the measured epochs of all rounds pooled per build -> min / median / max of ms per step. Saliency: the tool reports min /
median / max of its 6 calls; over the rounds min of the mins, median of the medians, max of the maxes. The bar per figure: the new
build's median <= the old build's median + the old build's own max - min. Exit status 1 if a figure misses it; a child that
fails ends the run at once (nothing further is started on the device)."""
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(cmd, env=None, limit=300):
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=limit, cwd=ROOT)
    if out.returncode != 0:
        print(f"{' '.join(cmd)} -> exit status {out.returncode}; stopping", flush=True)
        sys.exit(2)
    return json.loads(out.stdout.strip().splitlines()[-1])


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "n": len(v)}


def main():
    if sys.argv[1] == "--train-child":      # train_timing.py on another build of the library
        sys.path.insert(0, ROOT)
        from f2cnn_amd import build
        build.LIB_PATH = os.path.abspath(sys.argv[2])
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import train_timing
        return train_timing.main(sys.argv[3:])
    ap = argparse.ArgumentParser()
    ap.add_argument("old_lib")
    ap.add_argument("new_lib")
    ap.add_argument("out")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    libs = {"old": os.path.abspath(a.old_lib), "new": os.path.abspath(a.new_lib)}
    train = {k: {"32": [], "256": []} for k in libs}
    sal = {k: {} for k in libs}
    for r in range(a.rounds):
        for k, lib in libs.items():
            t = child([sys.executable, os.path.abspath(__file__), "--train-child", lib, "--only-hip", "--batches", "32,256", "--repeats", "2"])
            for b, e in t["batches"].items():
                steps = -(-65536 // int(b))
                train[k][b] += [1e3 * s / steps for s in e["hip"]["seconds"]]
            s = child([sys.executable, os.path.join(ROOT, "tools", "saliency_timing.py"), "--no-torch", "--reps", "3", "--warm", "1"],
                      env=dict(os.environ, F2CNN_PROBE_LIB=lib))
            for c in s["cases"]:
                for mem in ("host", "resident"):
                    sal[k].setdefault(f"{c['utterances']} utterances, hop {c['hop']}, {mem}", []).append(c[mem]["eval_saliency_batch_event_ms"])
            print(f"round {r + 1} {k} done", flush=True)
    result = {"method": __doc__, "rounds": a.rounds, "figures": {}}
    for b in ("32", "256"):
        result["figures"][f"f2_trainer_steps, batch {b}: ms per step"] = {k: spread(train[k][b]) for k in libs}
    for name in sal["old"]:
        result["figures"][f"f2_eval_saliency_batch, {name}: event ms"] = {
            k: {"min": min(p["min"] for p in sal[k][name]), "median": statistics.median(p["median"] for p in sal[k][name]),
                "max": max(p["max"] for p in sal[k][name]), "n": 6 * len(sal[k][name])} for k in libs}
    bad = 0
    for name, f in result["figures"].items():
        f["bar"] = f["old"]["median"] + f["old"]["max"] - f["old"]["min"]
        f["within_bar"] = f["new"]["median"] <= f["bar"]
        bad += not f["within_bar"]
        print(f"{name}: old {f['old']['min']:.4g} / {f['old']['median']:.4g} / {f['old']['max']:.4g}, new {f['new']['min']:.4g} / "
              f"{f['new']['median']:.4g} / {f['new']['max']:.4g}, bar {f['bar']:.4g}: {'within' if f['within_bar'] else 'MISSED'}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(result, fo, indent=1)
        fo.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
