"""16 utterances of 3 s (int16), 128 channels, at `--hop frame` (160), 16 and 1, from host memory:
(a) one f2_eval_segments_batch call (scores, labels, path, emissions, runs, tally come down);
(b) f2_eval_batch_strided alone - what the decoding adds is (a) - (b);
(c) the only other route: (b), then the sequential referee of tests/segments_referee.py on the host's scores (emissions in NumPy,
    the recurrence, the runs and the tally in interpreted Python).
Per repetition the HIP-event time between an event before the call and one after its last result, and the wall time; WARM unmeasured
repetitions, then REPS measured ones of (a) and (b) in alternating order, twice; (c) is measured REPS_REFEREE times (it takes
seconds at hop 1). The decoding launches' own share: the three stage calls on resident scores (device memory, nothing comes down but
value and run_offsets), by HIP events. (a)'s results are compared with (c)'s before anything is timed. Prints one JSON line; --out FILE
also writes it. Diagnostic."""
import argparse, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from f2cnn_amd import _lib, segments
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
import segments_referee as ref

ap = argparse.ArgumentParser()
ap.add_argument("--utterances", type=int, default=16)
ap.add_argument("--samples", type=int, default=48000)
ap.add_argument("--hops", default="160,16,1")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--reps-referee", type=int, default=2)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--out")
args = ap.parse_args()

C, FS, RADIUS, STEP = 128, 16000, 5, 160
B, n = args.utterances, args.samples
ctx = _lib.Context(0)
coefs = np.ascontiguousarray(filters.make_erb_filters(FS, filters.centre_freqs(FS, C, 100)), dtype=np.float64)
cnn = F2CNNModel.glorot(7).handle(ctx)
rng = np.random.default_rng(44)
wave = np.clip(np.round(rng.standard_normal(B * n) * 3000.0), -32768, 32767).astype(np.int16)
offsets = np.arange(B + 1, dtype=np.int64) * n
DSP = (coefs, B, C, False, 0.0, _lib.FFT_F32)
# forty "phonemes" of 75 ms per utterance, the same set for every utterance
edges = np.linspace(0, n, 41).astype(np.int64)
ivo = np.arange(B + 1, dtype=np.int64) * 40
ivb = np.tile(np.stack([edges[:-1], edges[1:]], axis=1), (B, 1))


def stat(t):
    return {"median": round(statistics.median(t), 3), "mean": round(statistics.fmean(t), 3),
            "stdev": round(statistics.stdev(t), 3) if len(t) > 1 else 0.0, "min": round(min(t), 3), "max": round(max(t), 3)}


e0, e1 = ctx.event(), ctx.event()


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    ev, wall = [], []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.record(e0)
        fn()
        ctx.record(e1)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(ctx.elapsed_ms(e0, e1))
    return ev, wall


result = {"utterances": B, "samples": n, "channels": C, "reps": 2 * args.reps, "reps_referee": args.reps_referee, "warm": args.warm,
          "path_tile": _lib.PATH_TILE, "cases": []}
for hop in [int(h) for h in args.hops.split(",")]:
    nw = _lib.strided_window_count(n, RADIUS, STEP, hop)
    N = B * nw
    wo = np.arange(B + 1, dtype=np.int64) * nw
    scale, penalty = segments.Quantise(hop, STEP, FS)
    EV = DSP + (RADIUS, STEP, hop)
    sc, lb = np.empty((N, 2), np.float32), np.empty(N, np.uint8)
    path, q, runs, tally = np.empty(N, np.uint8), np.empty(N, np.int32), np.empty((N, 4), np.int64), np.empty((len(ivb), 4), np.int64)
    sc_b, lb_b = np.empty_like(sc), np.empty_like(lb)
    host_ms = []
    dev = {k: ctx.malloc(max(a.nbytes, 8)) for k, a in (("sc", sc), ("lb", lb), ("path", path), ("q", q), ("runs", runs), ("tally", tally))}
    out = {}

    def fused():
        out["wo"], out["value"], out["ro"] = ctx.eval_segments_batch(cnn, wave, _lib.WAVE_I16, offsets, *EV, scale, penalty, ivo, ivb, sc, lb,
                                                                     path, q, runs, tally, _lib.MEM_HOST)

    def strided():
        ctx.eval_batch_strided(cnn, wave, _lib.WAVE_I16, offsets, *EV, sc_b, lb_b, _lib.MEM_HOST)

    def referee():
        strided()
        t0 = time.perf_counter()
        qr = ref.emissions(sc_b, scale)
        p, v = ref.decision_path(qr, wo, penalty)
        r = ref.decision_runs(p, qr, wo)
        t = ref.interval_tally(lb_b, p, qr, wo, ivo, ivb, RADIUS * STEP, hop)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        return qr, p, v, r, t

    def stages_resident():
        ctx.decision_path(dev["sc"], wo, scale, penalty, dev["path"], _lib.MEM_DEVICE, emissions=dev["q"])
        ctx.decision_runs(dev["path"], dev["q"], wo, dev["runs"], N, _lib.MEM_DEVICE)
        ctx.interval_tally(dev["lb"], dev["path"], dev["q"], wo, ivo, ivb, RADIUS * STEP, hop, dev["tally"], _lib.MEM_DEVICE)

    fused()
    qr, p, v, (ro_r, runs_r), t = referee()
    emissions_moved = int((qr != q).sum())      # a device log a few ulp from NumPy's can move an emission that stands on a half
    if emissions_moved == 0:
        assert np.array_equal(p, path) and np.array_equal(v, out["value"]) and np.array_equal(ro_r, out["ro"])
        assert np.array_equal(runs_r, runs[:len(runs_r)]) and np.array_equal(t, tally)
    host_ms.clear()
    ctx.h2d(dev["sc"], sc)
    ctx.h2d(dev["lb"], lb)

    a1, b1, a2, b2 = timed(fused, args.reps, args.warm), timed(strided, args.reps, args.warm), timed(fused, args.reps, args.warm), \
        timed(strided, args.reps, args.warm)
    c = timed(referee, args.reps_referee, 0)
    s = timed(stages_resident, 2 * args.reps, args.warm)
    fa, fb = stat(a1[0] + a2[0]), stat(b1[0] + b2[0])
    result["cases"].append({
        "hop": hop, "rows": int(N), "runs": int(out["ro"][-1]), "logit_scale": scale, "penalty": penalty, "emissions_moved": emissions_moved,
        "a_eval_segments_batch_event_ms": fa, "b_eval_batch_strided_event_ms": fb,
        "a_eval_segments_batch_wall_ms": stat(a1[1] + a2[1]), "b_eval_batch_strided_wall_ms": stat(b1[1] + b2[1]),
        "passes_event_ms_median": {"a": [stat(a1[0])["median"], stat(a2[0])["median"]], "b": [stat(b1[0])["median"], stat(b2[0])["median"]]},
        "a_minus_b_event_ms_median": round(fa["median"] - fb["median"], 3),
        "a_minus_b_over_b": round((fa["median"] - fb["median"]) / fb["median"], 4),
        "c_strided_plus_host_referee_wall_ms": stat(c[1]), "c_host_referee_alone_ms": stat(host_ms),
        "stage_calls_resident_event_ms": stat(s[0]), "stage_calls_resident_over_b": round(stat(s[0])["median"] / fb["median"], 4),
        "bytes_to_host": {"a": int(sc.nbytes + lb.nbytes + path.nbytes + q.nbytes + 32 * int(out["ro"][-1]) + tally.nbytes),
                          "b": int(sc.nbytes + lb.nbytes)}})
    ctx.synchronize()
    for ptr in dev.values():
        ctx.free(ptr)

print(json.dumps(result), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result) + "\n")
ctx.close()
