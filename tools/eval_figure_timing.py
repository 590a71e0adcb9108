"""16 utterances of 3 s (int16), 128 channels, figures of 1600 columns, at hop 160 and hop 1:
(a) one f2_eval_figure_batch call against (b) the only route to the same data there was before it - f2_eval_batch_strided, then
f2_gammatonegram_batch (a second filterbank + envelope pass), then the scores brought to the host and pooled to the columns in
NumPy. Both from host memory (wave up, everything down) and resident (wave, scores, labels, levels and track in device memory;
route (b) still has to download the scores to pool them). Per repetition the HIP-event time between an event recorded before the
first call and one recorded after the last result is there (the host's NumPy work of route (b) lies between the two, so it is
inside), and the wall time; WARM unmeasured repetitions, then REPS measured ones of each route in alternating order, twice.
Median, mean, standard deviation, min and max are reported, and the NumPy pooling's share on its own. The two routes' results
are compared before anything is timed. Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for saliency_timing.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel

ap = argparse.ArgumentParser()
ap.add_argument("--utterances", type=int, default=16)
ap.add_argument("--samples", type=int, default=48000)
ap.add_argument("--width", type=int, default=1600)
ap.add_argument("--hops", default="160,1")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--out")
args = ap.parse_args()

C, FS, RADIUS, STEP = 128, 16000, 5, 160
B, n, W = args.utterances, args.samples, args.width
ctx = _lib.Context(0)
coefs = np.ascontiguousarray(filters.make_erb_filters(FS, filters.centre_freqs(FS, C, 100)), dtype=np.float64)
model = F2CNNModel.glorot(7)
cnn = model.handle(ctx)
rng = np.random.default_rng(19)
wave = np.clip(np.round(rng.standard_normal(B * n) * 3000.0), -32768, 32767).astype(np.int16)
offsets = np.arange(B + 1, dtype=np.int64) * n
x = np.arange(W, dtype=np.int64)
lo, hi = x * n // W, (x + 1) * n // W
assert n >= W, "the NumPy route of this tool pools whole bins"
DSP = (coefs, B, C, False, 0.0, _lib.FFT_F32)


def numpy_track(scores, labels, nw, hop):
    """(B, W, 5) from the host scores: rows of a column are contiguous, so sums, minima and maxima are reduceat's"""
    out = np.full((B, W, 5), np.nan)
    t = RADIUS * STEP + hop * np.arange(nw, dtype=np.int64)
    j0, j1 = np.searchsorted(t, lo), np.searchsorted(t, hi)
    rows = j1 - j0
    full = rows > 0
    starts = j0[full]
    for b in range(B):
        p = scores[b * nw:(b + 1) * nw, 1]
        pd = p.astype(np.float64)
        out[b, :, 0] = rows
        out[b, :, 1] = 0
        end = j1[full][-1]
        out[b, full, 1] = np.add.reduceat((labels[b * nw:b * nw + end] != 0).astype(np.int64), starts)
        out[b, full, 2] = np.add.reduceat(pd[:end], starts) / rows[full]
        out[b, full, 3] = np.minimum.reduceat(p[:end], starts)
        out[b, full, 4] = np.maximum.reduceat(p[:end], starts)
    return out


def stat(t):
    return {"median": round(statistics.median(t), 3), "mean": round(statistics.fmean(t), 3), "stdev": round(statistics.stdev(t), 3),
            "min": round(min(t), 3), "max": round(max(t), 3)}


e0, e1 = ctx.event(), ctx.event()


def timed(fn):
    for _ in range(args.warm):
        fn()
    ev, wall = [], []
    for _ in range(args.reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.record(e0)
        fn()
        ctx.record(e1)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(ctx.elapsed_ms(e0, e1))
    return ev, wall


result = {"utterances": B, "samples": n, "channels": C, "width": W, "reps": 2 * args.reps, "warm": args.warm, "cases": []}
for hop in [int(h) for h in args.hops.split(",")]:
    nw = _lib.strided_window_count(n, RADIUS, STEP, hop)
    EV = DSP + (RADIUS, STEP, hop)
    sc, lb = np.empty((B * nw, 2), np.float32), np.empty(B * nw, np.uint8)
    lv, tr = np.zeros((B, C, W), np.uint8), np.empty((B, W, 5))
    sc_p, lb_p, lv_p = np.empty_like(sc), np.empty_like(lb), np.zeros_like(lv)
    pool_ms = []
    dev = {k: ctx.malloc(max(a.nbytes, 8)) for k, a in (("wave", wave), ("sc", sc), ("lb", lb), ("lv", lv), ("tr", tr))}
    ctx.h2d(dev["wave"], wave)

    def fused_host():
        ctx.eval_figure_batch(cnn, wave, _lib.WAVE_I16, offsets, *EV, None, W, 0, lv, tr, sc, lb, _lib.MEM_HOST)

    def parent_host():
        ctx.eval_batch_strided(cnn, wave, _lib.WAVE_I16, offsets, *EV, sc_p, lb_p, _lib.MEM_HOST)
        ctx.gammatonegram_batch(wave, _lib.WAVE_I16, offsets, *DSP, None, W, 0, None, lv_p, _lib.MEM_HOST)
        t0 = time.perf_counter()
        out = numpy_track(sc_p, lb_p, nw, hop)
        pool_ms.append((time.perf_counter() - t0) * 1e3)
        return out

    def fused_resident():
        ctx.eval_figure_batch(cnn, dev["wave"], _lib.WAVE_I16, offsets, *EV, None, W, 0, dev["lv"], dev["tr"], dev["sc"], dev["lb"],
                              _lib.MEM_DEVICE)

    def parent_resident():
        ctx.eval_batch_strided(cnn, dev["wave"], _lib.WAVE_I16, offsets, *EV, dev["sc"], dev["lb"], _lib.MEM_DEVICE)
        ctx.gammatonegram_batch(dev["wave"], _lib.WAVE_I16, offsets, *DSP, None, W, 0, None, dev["lv"], _lib.MEM_DEVICE)
        ctx.d2h(sc_p, dev["sc"])
        ctx.d2h(lb_p, dev["lb"])
        return numpy_track(sc_p, lb_p, nw, hop)

    # the two routes give the same data: scores and labels bit for bit, the track up to the mean's summation order, the levels
    # up to a level where the spectral route's envelopes differ in the last bits
    fused_host()
    want = parent_host()
    assert np.array_equal(sc.view(np.uint8), sc_p.view(np.uint8)) and np.array_equal(lb, lb_p)
    for k in (0, 1, 3, 4):
        assert np.array_equal(tr[..., k], want[..., k], equal_nan=True), k
    assert np.allclose(tr[..., 2], want[..., 2], rtol=1e-12, atol=0, equal_nan=True)
    level_diff = np.abs(lv.astype(np.int64) - lv_p.astype(np.int64))
    assert level_diff.max() <= 1, level_diff.max()
    fused_resident()
    tr_d = np.empty_like(tr)
    ctx.synchronize()
    ctx.d2h(tr_d, dev["tr"])
    assert tr_d.tobytes() == tr.tobytes()
    pool_ms.clear()

    case = {"hop": hop, "windows": int(B * nw), "levels_differing_by_one": int((level_diff == 1).sum())}
    for name, a, b in (("host", fused_host, parent_host), ("resident", fused_resident, parent_resident)):
        a1, b1, a2, b2 = timed(a), timed(b), timed(a), timed(b)       # alternate: neither owns the warmer half of the run
        fa, pa = stat(a1[0] + a2[0]), stat(b1[0] + b2[0])
        case[name] = {"eval_figure_batch_event_ms": fa, "strided_plus_gammatonegram_plus_numpy_event_ms": pa,
                      "eval_figure_batch_wall_ms": stat(a1[1] + a2[1]), "strided_plus_gammatonegram_plus_numpy_wall_ms": stat(b1[1] + b2[1]),
                      "passes_event_ms_median": {"eval_figure_batch": [stat(a1[0])["median"], stat(a2[0])["median"]],
                                                 "parent": [stat(b1[0])["median"], stat(b2[0])["median"]]},
                      "ratio_parent_over_fused_median": round(pa["median"] / fa["median"], 3)}
    case["numpy_pooling_ms"] = stat(pool_ms)
    case["bytes_to_host_resident"] = {"eval_figure_batch": 0, "parent": int(sc.nbytes + lb.nbytes)}
    result["cases"].append(case)
    ctx.synchronize()
    for p in dev.values():
        ctx.free(p)

print(json.dumps(result), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result) + "\n")
ctx.close()
