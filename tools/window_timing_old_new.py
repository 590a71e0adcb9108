"""Renders and validation-set calls of two builds of the library, alternated (profiles/r42_a_window_timing_old_new.json):
tools/train_augment_timing.py, train_rooms_timing.py, train_colours_timing.py and train_smear_timing.py (each --passes 1, the stage
kernels alone cut to a token size: they are not what is compared) and the four validation-set calls of `cnn train --from-wav`
(f2_input_batch_noisy / _wet / _coloured / _smeared on one group of 64 files of 3 s in host memory, 164 centres a file, median of 5
after a warm call), each in a process of its own per build (F2CNN_PROBE_LIB, as tools/figure_timing_old_new.py selects a build), the
builds alternating: old, new, old, new, ...

    python3 tools/window_timing_old_new.py OLD_LIB NEW_LIB OUT.json [--rounds 3] [--utterances 200]

A figure is every median a tool reports for a render (host seconds and HIP-event ms) and every validation-set call. Per figure the
old build's values over the rounds give its spread; the new build passes where its median over the rounds is not above the old
build's largest value ("inside": also not below its smallest). Exit status 1 if a figure lies above; a child that fails ends the
run at once (nothing further is started on the device)."""
import argparse, json, os, re, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIGURE = re.compile(r"render.*\.(median_s|host_median_s|device_median_ms|render_device_ms)$|^validation\.")


def validation_child():
    """the four validation-set calls as Training._render_windows makes them, one JSON line"""
    import numpy as np
    from f2cnn_amd import _lib, build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
    from f2cnn_amd.gammatone import filters
    B, n, per, C, radius, step = 64, 48000, 164, 128, 5, 160
    rng = np.random.default_rng(3)
    flat = (rng.standard_normal(B * n) * 3000).astype(np.int16)
    offsets, coff = np.arange(B + 1, dtype=np.int64) * n, np.arange(B + 1, dtype=np.int64) * per
    cen = np.tile(np.linspace(radius * step, n - 1 - radius * step, per).astype(np.int64), B)
    freqs = filters.centre_freqs(16000, C, 100)
    coefs = np.ascontiguousarray(filters.make_erb_filters(16000, freqs), dtype=np.float64)
    rirs = [rng.standard_normal(t) * np.exp(-np.arange(t) / (t / 5.0)) for t in (3200, 6400)]
    firs = [h / np.sqrt(h @ h) for h in (rng.standard_normal(1025) for _ in range(2))]
    mix = np.abs(np.subtract.outer(np.arange(C), np.arange(C))) < 4
    mix = (mix / mix.sum(axis=1, keepdims=True))[None]
    room, lev, out = np.full(B, 1, np.int32), np.full(B, 0, np.int32), np.empty((B * per, 2 * radius + 1, C), np.float32)
    ctx = _lib.default_context()
    front = (flat, _lib.WAVE_I16, offsets, coefs, B, C, False, 0.0, _lib.FFT_F32, coff, cen, radius, step, True)
    calls = {"input_batch_noisy": lambda: ctx.input_batch_noisy(*front, (20.0, 10.0), lev, 0, 7, out, _lib.MEM_HOST),
             "input_batch_wet": lambda: ctx.input_batch_wet(*front, rirs, room, (20.0, 10.0), lev, 0, 7, out, _lib.MEM_HOST),
             "input_batch_coloured": lambda: ctx.input_batch_coloured(*front, rirs, room, (20.0, 10.0), firs, lev, 0, 7, out, _lib.MEM_HOST),
             "input_batch_smeared": lambda: ctx.input_batch_smeared(*front, rirs, room, (20.0, 10.0), firs, lev, 0, 7, mix, np.zeros(B, np.int32),
                                                                    out, _lib.MEM_HOST)}
    got = {k: [] for k in calls}
    for r in range(6):
        for k, fn in calls.items():                                         # alternating; round 0 warms
            t0 = time.perf_counter()
            fn()
            if r:
                got[k].append(time.perf_counter() - t0)
    print(json.dumps({"validation": {k: statistics.median(v) for k, v in got.items()}}))
    return 0


def augment_child(argv):
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_augment_timing
    return train_augment_timing.main(argv)


def leaves(node, path=""):
    if isinstance(node, dict):
        for k, v in node.items():
            yield from leaves(v, f"{path}.{k}" if path else str(k))
    elif isinstance(node, list):
        for i, v in enumerate(node):
            yield from leaves(v, f"{path}.{i}")
    elif isinstance(node, (int, float)) and not isinstance(node, bool):
        yield path, float(node)


def main():
    if sys.argv[1] == "--validation-child":
        return validation_child()
    if sys.argv[1] == "--augment-child":
        return augment_child(sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("old_lib")
    ap.add_argument("new_lib")
    ap.add_argument("out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--utterances", type=int, default=200)
    a = ap.parse_args()
    me, tool = os.path.abspath(__file__), lambda name: os.path.join(ROOT, "tools", name)
    size = ["--utterances", str(a.utterances), "--passes", "1"]
    token = ["--kernel-utterances", "8", "--kernel-reps", "4"]
    children = {"train_augment_timing": [me, "--augment-child"] + size + ["--batches", "256"],
                "train_rooms_timing": [tool("train_rooms_timing.py")] + size + token + ["--batches", "256"],
                "train_colours_timing": [tool("train_colours_timing.py")] + size + token,
                "train_smear_timing": [tool("train_smear_timing.py")] + size + token,
                "validation": [me, "--validation-child"]}
    values = {"old": {}, "new": {}}
    for r in range(a.rounds):
        for build, lib in (("old", a.old_lib), ("new", a.new_lib)):
            for name, cmd in children.items():
                out = subprocess.run([sys.executable] + cmd, env=dict(os.environ, F2CNN_PROBE_LIB=os.path.abspath(lib)), stdout=subprocess.PIPE,
                                     text=True, timeout=400, cwd=ROOT)
                if out.returncode != 0:
                    print(f"{name} with the {build} build -> exit status {out.returncode}; stopping\n{out.stdout[-2000:]}", flush=True)
                    return 2
                last = out.stdout.strip().splitlines()[-1]
                for path, v in leaves(json.loads(last[last.index("{"):])):
                    if FIGURE.search(path):
                        values[build].setdefault(f"{name}: {path}", []).append(v)
                print(f"round {r + 1} {build} {name} done", flush=True)
    result = {"method": __doc__, "rounds": a.rounds, "utterances": a.utterances, "figures": {}}
    above = 0
    for fig, old in values["old"].items():
        new = values["new"][fig]
        med = statistics.median(new)
        where = "above" if med > max(old) else "below" if med < min(old) else "inside"
        above += where == "above"
        result["figures"][fig] = {"old": old, "new": new, "old_min": min(old), "old_max": max(old), "new_median": med, "new_median_is": where}
        print(f"{fig}: old {min(old):.6g} .. {max(old):.6g}, new median {med:.6g}: {where}", flush=True)
    print(f"{len(values['old']) - above} of {len(values['old'])} figures not above the old build's spread", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    return 1 if above else 0


if __name__ == "__main__":
    sys.exit(main())
