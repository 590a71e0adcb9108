"""16 utterances of 3 s (int16), 128 channels, 16 bands of 8 channels (L = 17 levels), maps of 1600 columns, at hop 160 and hop 16:
(a) one f2_eval_occlusion_batch call against (b) the only route to the same data there was before it - f2_input_batch brings the
normalised windows to the host, NumPy makes the 16 blanked copies of every window, f2_cnn_forward takes all 17 n windows back up
from host memory, NumPy reduces the scores to map and summary - and (c) f2_eval_batch_strided alone, so that the cost per level
shows against L = 17. From host memory (wave up, everything down) and resident (wave and every result of (a) and (c) in device
memory; route (b) takes the wave from device memory and the windows from the host, it has no other way). Per repetition the
HIP-event time between an event recorded before the first call and one recorded after the last result is there (the host's NumPy
work of route (b) lies between the two, so it is inside), and the wall time; WARM unmeasured repetitions, then REPS measured ones
of each route in alternating order, twice. The routes' results are compared before anything is timed. Prints one JSON line; --out
FILE also writes it. --only-fused runs route (a) alone, resident: the command to put behind `rocprofv3 --kernel-trace --stats` for
k_occlude_windows' time and its share of the call. Diagnostic."""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for saliency_timing.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.scripts.CNN.Evaluating import OcclusionPatches

ap = argparse.ArgumentParser()
ap.add_argument("--utterances", type=int, default=16)
ap.add_argument("--samples", type=int, default=48000)
ap.add_argument("--width", type=int, default=1600)
ap.add_argument("--band", type=int, default=8)
ap.add_argument("--hops", default="160,16")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--only-fused", action="store_true",
                help="run only route (a), resident, REPS times per hop: the command for a kernel trace of the fused call")
ap.add_argument("--out")
args = ap.parse_args()

C, FS, RADIUS, STEP, R = 128, 16000, 5, 160, 11
B, n, W = args.utterances, args.samples, args.width
ctx = _lib.Context(0)
coefs = np.ascontiguousarray(filters.make_erb_filters(FS, filters.centre_freqs(FS, C, 100)), dtype=np.float64)
model = F2CNNModel.glorot(7)
cnn = model.handle(ctx)
rng = np.random.default_rng(20)
wave = np.clip(np.round(rng.standard_normal(B * n) * 3000.0), -32768, 32767).astype(np.int16)
offsets = np.arange(B + 1, dtype=np.int64) * n
patches = OcclusionPatches(R, C, args.band, args.band)
K = len(patches)
L = K + 1
x = np.arange(W, dtype=np.int64)
lo, hi = x * n // W, (x + 1) * n // W
assert n >= W, "the NumPy route of this tool pools whole bins"
DSP = (coefs, B, C, False, 0.0, _lib.FFT_F32)


def numpy_map(scores, labels, nw, hop):
    """(B, K, W, 4) and (B, K, 4) from the host scores (B nw, L, 2) and labels (B nw, L): rows of a column are contiguous"""
    t = RADIUS * STEP + hop * np.arange(nw, dtype=np.int64)
    j0, j1 = np.searchsorted(t, lo), np.searchsorted(t, hi)
    rows = j1 - j0
    full = rows > 0
    starts, end = j0[full], j1[full][-1]
    p = scores[..., 1].astype(np.float64).reshape(B, nw, L)
    d = p[:, :, 1:] - p[:, :, :1]
    lab = (labels != 0).reshape(B, nw, L)
    flip = (lab[:, :, 1:] != lab[:, :, :1]).astype(np.int64)
    out = np.full((B, K, W, 4), np.nan)
    out[..., 0] = rows
    out[..., 1] = 0
    out[:, :, full, 1] = np.add.reduceat(flip[:, :end], starts, axis=1).transpose(0, 2, 1)
    out[:, :, full, 2] = np.add.reduceat(d[:, :end], starts, axis=1).transpose(0, 2, 1) / rows[full]
    out[:, :, full, 3] = np.add.reduceat(np.abs(d[:, :end]), starts, axis=1).transpose(0, 2, 1) / rows[full]
    summary = np.stack([np.full((B, K), float(nw)), flip.sum(axis=1), d.sum(axis=1) / nw, np.abs(d).sum(axis=1) / nw], axis=2)
    return out, summary


def numpy_occlude(windows):
    occ = np.repeat(windows[:, None], L, axis=1)
    for k, (r0, r1, c0, c1) in enumerate(patches):
        occ[:, k + 1, r0:r1, c0:c1] = 0.0
    return occ


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


result = {"utterances": B, "samples": n, "channels": C, "width": W, "patches": K, "levels": L, "reps": 2 * args.reps, "warm": args.warm,
          "cases": []}
for hop in [int(h) for h in args.hops.split(",")]:
    nw = _lib.strided_window_count(n, RADIUS, STEP, hop)
    N = B * nw
    EV = DSP + (RADIUS, STEP, hop)
    sc, lb = np.empty((N, L, 2), np.float32), np.empty((N, L), np.uint8)
    mp, sm = np.empty((B, K, W, 4)), np.empty((B, K, 4))
    sc0, lb0 = np.empty((N, 2), np.float32), np.empty(N, np.uint8)
    windows = np.empty((N, R, C), np.float32)
    sc_p, lb_p = np.empty_like(sc), np.empty_like(lb)
    centre_offsets = np.arange(B + 1, dtype=np.int64) * nw
    centres = np.tile(RADIUS * STEP + hop * np.arange(nw, dtype=np.int64), B)
    host_ms = {"occlude": [], "reduce": []}
    dev = {k: ctx.malloc(max(a.nbytes, 8)) for k, a in (("wave", wave), ("sc", sc), ("lb", lb), ("mp", mp), ("sm", sm), ("sc0", sc0),
                                                        ("lb0", lb0), ("win", windows))}
    ctx.h2d(dev["wave"], wave)

    def fused_host():
        ctx.eval_occlusion_batch(cnn, wave, _lib.WAVE_I16, offsets, *EV, patches, 0.0, None, W, 0, None, mp, sm, sc, lb, _lib.MEM_HOST)

    def fused_resident():
        ctx.eval_occlusion_batch(cnn, dev["wave"], _lib.WAVE_I16, offsets, *EV, patches, 0.0, None, W, 0, None, dev["mp"], dev["sm"],
                                 dev["sc"], dev["lb"], _lib.MEM_DEVICE)

    def parent_tail():
        t0 = time.perf_counter()
        occ = numpy_occlude(windows)
        t1 = time.perf_counter()
        ctx.cnn_forward(cnn, occ.reshape(-1, R, C), N * L, sc_p, lb_p, _lib.MEM_HOST)
        t2 = time.perf_counter()
        out = numpy_map(sc_p, lb_p, nw, hop)
        host_ms["occlude"].append((t1 - t0) * 1e3)
        host_ms["reduce"].append((time.perf_counter() - t2) * 1e3)
        return out

    def parent_host():
        ctx.input_batch(wave, _lib.WAVE_I16, offsets, *DSP, centre_offsets, centres, RADIUS, STEP, True, windows, _lib.MEM_HOST)
        return parent_tail()

    def parent_resident():
        ctx.input_batch(dev["wave"], _lib.WAVE_I16, offsets, *DSP, centre_offsets, centres, RADIUS, STEP, True, dev["win"], _lib.MEM_DEVICE)
        ctx.synchronize()
        ctx.d2h(windows, dev["win"])
        return parent_tail()

    def strided_host():
        ctx.eval_batch_strided(cnn, wave, _lib.WAVE_I16, offsets, *EV, sc0, lb0, _lib.MEM_HOST)

    def strided_resident():
        ctx.eval_batch_strided(cnn, dev["wave"], _lib.WAVE_I16, offsets, *EV, dev["sc0"], dev["lb0"], _lib.MEM_DEVICE)

    if args.only_fused:
        for _ in range(args.warm + args.reps):
            fused_resident()
        ctx.synchronize()
        result["cases"].append({"hop": hop, "windows": int(N), "level_windows": int(N * L), "fused_resident_calls": args.warm + args.reps})
        for p in dev.values():
            ctx.free(p)
        continue

    # the routes give the same data: scores and labels bit for bit, counts exactly, the means up to the summation order
    fused_host()
    want_map, want_summary = parent_host()
    strided_host()
    assert np.array_equal(sc.view(np.uint8), sc_p.view(np.uint8)) and np.array_equal(lb, lb_p)
    assert np.array_equal(sc[:, 0].copy().view(np.uint8), sc0.view(np.uint8)) and np.array_equal(lb[:, 0], lb0)
    for got, want in ((mp, want_map), (sm, want_summary)):
        assert np.array_equal(got[..., :2], want[..., :2])
        assert np.allclose(got[..., 2:], want[..., 2:], rtol=1e-9, atol=1e-15, equal_nan=True)
    fused_resident()
    mp_d = np.empty_like(mp)
    ctx.synchronize()
    ctx.d2h(mp_d, dev["mp"])
    assert mp_d.tobytes() == mp.tobytes()
    for v in host_ms.values():
        v.clear()

    case = {"hop": hop, "windows": int(N), "level_windows": int(N * L)}
    for name, a, b, c in (("host", fused_host, parent_host, strided_host), ("resident", fused_resident, parent_resident, strided_resident)):
        a1, b1, c1, a2, b2, c2 = timed(a), timed(b), timed(c), timed(a), timed(b), timed(c)     # alternate: no route owns the warmer half
        fa, pa, sa = stat(a1[0] + a2[0]), stat(b1[0] + b2[0]), stat(c1[0] + c2[0])
        case[name] = {"eval_occlusion_batch_event_ms": fa, "input_numpy_forward_numpy_event_ms": pa, "eval_batch_strided_event_ms": sa,
                      "eval_occlusion_batch_wall_ms": stat(a1[1] + a2[1]), "input_numpy_forward_numpy_wall_ms": stat(b1[1] + b2[1]),
                      "eval_batch_strided_wall_ms": stat(c1[1] + c2[1]),
                      "passes_event_ms_median": {"eval_occlusion_batch": [stat(a1[0])["median"], stat(a2[0])["median"]],
                                                 "parent": [stat(b1[0])["median"], stat(b2[0])["median"]],
                                                 "strided": [stat(c1[0])["median"], stat(c2[0])["median"]]},
                      "ratio_parent_over_fused_median": round(pa["median"] / fa["median"], 3),
                      "ratio_fused_over_strided_median": round(fa["median"] / sa["median"], 3)}
    case["numpy_ms"] = {k: stat(v) for k, v in host_ms.items()}
    case["bytes_over_the_link_resident"] = {"eval_occlusion_batch": 0, "parent": int(windows.nbytes * (L + 1) + sc.nbytes + lb.nbytes)}
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
