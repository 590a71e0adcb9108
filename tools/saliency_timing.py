"""1 and 16 utterances of 3 s (int16), 128 channels, a decision per frame (hop 160) and hop 16, from host memory and resident:
one f2_eval_saliency_batch call (map of 1600 columns and summary) against
  (a) f2_eval_batch_strided alone - a plain evaluation; with --parent-lib LIB also in a fresh process on that build of the library
      (the parent commit's: `git archive` it, `python -m f2cnn_amd.build` there),
  (b) f2_eval_occlusion_batch at 1:1 (128 bands of one channel, L = 129 levels), the only per-channel answer there was,
  (c) PyTorch-ROCm autograd of scripts/CNN/Training.py's build_network on the same normalised windows (f2_input_batch leaves them in
      device memory for the library's resident route; torch gets them as a device tensor, NCHW, and returns dP(rising)/dx), the only
      backward pass there was. (c) is timed without the filterbank, the envelopes and the windows: forward + backward alone.
Per repetition the HIP-event time between an event recorded before the call and one recorded after it, and the wall time; WARM
unmeasured repetitions, then REPS measured ones of each route in alternating order, twice (tools/occlusion_timing.py's scheme). The
gradients of (c) and of f2_cnn_input_gradient are compared before anything is timed.
--only-gradient N runs f2_cnn_input_gradient on N resident windows WARM + REPS times and nothing else: the command to put behind
`rocprofv3 --kernel-trace --stats`; --kernel-stats CSV then folds that run's per-kernel times into the result, each against the
multiply-adds and the bytes the kernel has to move (share of the 157.3 TFLOP/s f32 matrix peak, of the 8 TB/s HBM peak).
Prints one JSON line; --out FILE also writes it. Diagnostic."""
import argparse, csv, json, os, statistics, subprocess, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):   # another build of the library, as for noise_sweep_timing.py
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel

ap = argparse.ArgumentParser()
ap.add_argument("--utterances", default="1,16")
ap.add_argument("--samples", type=int, default=48000)
ap.add_argument("--width", type=int, default=1600)
ap.add_argument("--hops", default="160,16")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warm", type=int, default=1)
ap.add_argument("--parent-lib", help="another build of the library: route (a) is also timed on it, in a process of its own")
ap.add_argument("--only-strided", action="store_true", help="route (a) alone (what --parent-lib starts)")
ap.add_argument("--only-gradient", type=int, metavar="N", help="f2_cnn_input_gradient on N resident windows, for a kernel trace")
ap.add_argument("--kernel-stats", help="kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of --only-gradient N")
ap.add_argument("--kernel-stats-windows", type=int, default=0, help="the N of that run")
ap.add_argument("--kernel-stats-calls", type=int, default=0, help="its WARM + REPS")
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--out")
args = ap.parse_args()

C, FS, RADIUS, STEP, R = 128, 16000, 5, 160, 11
n, W = args.samples, args.width
MFMA_PEAK, HBM_PEAK = 157.3e12, 8.0e12


def stat(t):
    return {"median": round(statistics.median(t), 3), "mean": round(statistics.fmean(t), 3), "stdev": round(statistics.stdev(t), 3) if len(t) > 1 else 0.0,
            "min": round(min(t), 3), "max": round(max(t), 3)}


def chain_work(nwin):
    """{kernel name pattern: (multiply-adds, bytes it has to move)} of the chain for nwin 11 x 128 windows"""
    H1, W1, H2, W2, Hp1, Wp1, H4, W4, Hp2, Wp2 = R, C, R - 2, C - 2, (R - 2) // 2, (C - 2) // 2, (R - 2) // 2 - 2, (C - 2) // 2 - 2, \
        ((R - 2) // 2 - 2) // 2, ((C - 2) // 2 - 2) // 2
    flat = Hp2 * Wp2 * 64
    f = 4 * nwin
    a1, a2, p1, a3, a4 = H1 * W1 * 32, H2 * W2 * 32, Hp1 * Wp1 * 32, Hp1 * Wp1 * 64, H4 * W4 * 64
    return {
        "k_conv1_fwd": (nwin * H1 * W1 * 9 * 32, f * (H1 * W1 + a1)),
        "k_conv3x3_f32<32, 32, 0, 0, 0": (nwin * H2 * W2 * 9 * 32 * 32, f * (a1 + a2)),
        "k_pool2x2": (0, None),
        "k_conv3x3_f32<32, 64, 1, 0, 0": (nwin * Hp1 * Wp1 * 9 * 32 * 64, f * (p1 + a3)),
        "k_conv3x3_f32<64, 64, 0, 0, 0": (nwin * H4 * W4 * 9 * 64 * 64, f * (a3 + a4)),
        "k_dense1_mfma": (nwin * flat * 544, f * (flat + 516)),
        "k_dense2_softmax": (nwin * 516 * 2, f * 518),
        "k_grad_dense2": (nwin * 516, f * (516 + 576)),
        "k_gemm_rows": (nwin * 576 * flat, f * (576 + flat)),
        "k_conv3x3_f32<64, 64, 2, 1, 1": (nwin * Hp1 * Wp1 * 9 * 64 * 64, f * (flat + a4 + 2 * a3)),
        "k_conv3x3_f32<64, 32, 1, 0, 2": (nwin * Hp1 * Wp1 * 9 * 64 * 32, f * (a3 + p1)),
        "k_conv3x3_f32<32, 32, 2, 1, 1": (nwin * H1 * W1 * 9 * 32 * 32, f * (p1 + a2 + 2 * a1)),
        "k_conv1_bwd": (nwin * H1 * W1 * 9 * 32, f * (a1 + H1 * W1)),
        "k_grad_profile": (0, nwin * (8 * H1 * W1 + 16 * W1)),
    }


def fold_kernel_stats(path, nwin, calls):
    rows = list(csv.DictReader(open(path)))
    work = chain_work(nwin)
    pool_bytes = 4 * nwin * ((R - 2) * (C - 2) * 32 * 1.25 + ((R - 2) // 2 - 2) * ((C - 2) // 2 - 2) * 64 * 1.25)
    out, total = [], 0.0
    def mangled(k):      # "k_conv3x3_f32<32, 32, 0, 0, 0" as the statistics name it when they keep the mangled symbol
        if "<" not in k:
            return k
        base, params = k.split("<")
        return base + "I" + "".join("Li{}E".format(p.strip()) for p in params.split(","))

    for r in rows:
        name = r["Name"]
        hit = [k for k in work if k in name or mangled(k) in name]
        if not hit:
            continue
        macs, nbytes = work[hit[0]]
        if nbytes is None:
            nbytes = pool_bytes          # (the two pool launches share a name: their bytes together)
        ms = float(r["TotalDurationNs"]) / 1e6 / calls
        total += ms
        flops = 2.0 * macs / (ms * 1e-3)
        out.append({"kernel": hit[0] + (">" if "<" in hit[0] else ""), "launches_per_call": int(r["Calls"]) / calls, "ms_per_call": round(ms, 4),
                    "tflops": round(flops / 1e12, 2), "share_of_f32_mfma_peak": round(flops / MFMA_PEAK, 4),
                    "required_GB": round(nbytes / 1e9, 4), "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)})
    return {"windows": nwin, "calls": calls, "chain_ms_per_call": round(total, 3), "windows_per_s": round(nwin / (total * 1e-3)), "kernels": out}


ctx = _lib.Context(0)
coefs = np.ascontiguousarray(filters.make_erb_filters(FS, filters.centre_freqs(FS, C, 100)), dtype=np.float64)
DSP = (coefs, C, False, 0.0, _lib.FFT_F32)
rng = np.random.default_rng(20)
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


net = None
if not (args.only_strided or args.only_gradient or args.no_torch):
    import torch
    from f2cnn_amd.scripts.CNN.Training import build_network
    torch.manual_seed(7)
    net = build_network(R, C).eval()
    model = F2CNNModel.from_torch_state_dict(net.state_dict(), R, C)
    net = net.cuda()
else:
    model = F2CNNModel.glorot(7)
cnn = model.handle(ctx)
result = {"samples": n, "channels": C, "width": W, "reps": 2 * args.reps, "warm": args.warm, "cases": []}

if args.only_gradient:
    N = args.only_gradient
    x = rng.random((N, R, C)).astype(np.float32)
    d_x, d_g, d_p = ctx.malloc(x.nbytes), ctx.malloc(x.nbytes), ctx.malloc(16 * C * N)
    ctx.h2d(d_x, x)
    ev, wall = timed(lambda: ctx.cnn_input_gradient(cnn, d_x, N, d_g, d_p, None, _lib.MEM_DEVICE))
    result["only_gradient"] = {"windows": N, "calls": args.warm + args.reps, "event_ms": stat(ev), "windows_per_s": round(N / (statistics.median(ev) * 1e-3))}
    for p in (d_x, d_g, d_p):
        ctx.free(p)
else:
    for B in [int(b) for b in args.utterances.split(",")]:
        wave = np.clip(np.round(rng.standard_normal(B * n) * 3000.0), -32768, 32767).astype(np.int16)
        offsets = np.arange(B + 1, dtype=np.int64) * n
        for hop in [int(h) for h in args.hops.split(",")]:
            nw = _lib.strided_window_count(n, RADIUS, STEP, hop)
            N = B * nw
            EV = (DSP[0], B) + DSP[1:] + (RADIUS, STEP, hop)
            sc, lb = np.empty((N, 2), np.float32), np.empty(N, np.uint8)
            case = {"utterances": B, "hop": hop, "windows": int(N), "audio_s": B * n / FS}
            d_wave, d_sc, d_lb = ctx.malloc(wave.nbytes), ctx.malloc(sc.nbytes), ctx.malloc(max(lb.nbytes, 8))
            ctx.h2d(d_wave, wave)
            strided = {"host": lambda: ctx.eval_batch_strided(cnn, wave, _lib.WAVE_I16, offsets, *EV, sc, lb, _lib.MEM_HOST),
                       "resident": lambda: ctx.eval_batch_strided(cnn, d_wave, _lib.WAVE_I16, offsets, *EV, d_sc, d_lb, _lib.MEM_DEVICE)}
            if args.only_strided:
                for name, fn in strided.items():
                    a1, a2 = timed(fn), timed(fn)
                    case[name] = {"eval_batch_strided_event_ms": stat(a1[0] + a2[0]), "eval_batch_strided_wall_ms": stat(a1[1] + a2[1])}
                result["cases"].append(case)
                for p in (d_wave, d_sc, d_lb):
                    ctx.free(p)
                continue
            K = C
            patches = np.array([[0, R, c, c + 1] for c in range(C)], np.int32)
            mp, sm = np.empty((B, C, W, 3)), np.empty((B, C, 3))
            omp, osm = np.empty((B, K, W, 4)), np.empty((B, K, 4))
            d_mp, d_sm, d_omp, d_osm = ctx.malloc(mp.nbytes), ctx.malloc(sm.nbytes), ctx.malloc(omp.nbytes), ctx.malloc(osm.nbytes)
            sal = {"host": lambda: ctx.eval_saliency_batch(cnn, wave, _lib.WAVE_I16, offsets, *EV, None, W, 0, None, mp, sm, sc, lb, _lib.MEM_HOST),
                   "resident": lambda: ctx.eval_saliency_batch(cnn, d_wave, _lib.WAVE_I16, offsets, *EV, None, W, 0, None, d_mp, d_sm, d_sc, d_lb,
                                                               _lib.MEM_DEVICE)}
            # (the occlusion call's scores of all 129 levels stay in its scratch: maps and summary out, as for the saliency call)
            occ = {"host": lambda: ctx.eval_occlusion_batch(cnn, wave, _lib.WAVE_I16, offsets, *EV, patches, 0.0, None, W, 0, None, omp, osm, None,
                                                            None, _lib.MEM_HOST),
                   "resident": lambda: ctx.eval_occlusion_batch(cnn, d_wave, _lib.WAVE_I16, offsets, *EV, patches, 0.0, None, W, 0, None, d_omp, d_osm,
                                                                None, None, _lib.MEM_DEVICE)}
            # the windows, resident, for (c) and for the comparison of the two backward passes
            centre_offsets = np.arange(B + 1, dtype=np.int64) * nw
            centres = np.tile(RADIUS * STEP + hop * np.arange(nw, dtype=np.int64), B)
            windows = np.empty((N, R, C), np.float32)
            ctx.input_batch(wave, _lib.WAVE_I16, offsets, DSP[0], B, *DSP[1:], centre_offsets, centres, RADIUS, STEP, True, windows, _lib.MEM_HOST)
            sal["host"]()
            occ["host"]()
            with np.errstate(invalid="ignore"):
                case["first_order_check"] = {"corr_sumGx_vs_minus_occlusion_d": round(float(np.corrcoef(sm[..., 1].ravel(), -osm[..., 2].ravel())[0, 1]), 4)}
            if net is not None:
                xt = torch.from_numpy(windows).cuda()[:, None]
                CH = 4096

                def autograd():
                    grads = []
                    for s in range(0, N, CH):
                        xs = xt[s:s + CH].detach().requires_grad_(True)
                        torch.softmax(net(xs), dim=1)[:, 1].sum().backward()
                        grads.append(xs.grad)
                    torch.cuda.synchronize()
                    return grads

                G = np.empty((N, R, C), np.float32)
                ctx.cnn_input_gradient(cnn, windows, N, G, None, None, _lib.MEM_HOST)
                Gt = torch.cat(autograd())[:, 0].cpu().numpy()
                scale = np.abs(Gt).reshape(N, -1).max(axis=1)
                err = np.abs(G - Gt).reshape(N, -1).max(axis=1) / np.maximum(scale, 1e-30)
                case["device_vs_torch_autograd"] = {"median_rel_err": float(np.median(err)), "windows_beyond_5e-6": int((err > 5e-6).sum())}
                d_x, d_g = ctx.malloc(windows.nbytes), ctx.malloc(windows.nbytes)
                ctx.h2d(d_x, windows)
                lib_grad = lambda: ctx.cnn_input_gradient(cnn, d_x, N, d_g, None, None, _lib.MEM_DEVICE)
                g1, t1, g2, t2 = timed(lib_grad), timed(autograd), timed(lib_grad), timed(autograd)
                lg, tg = stat(g1[1] + g2[1]), stat(t1[1] + t2[1])      # wall: torch's work is on its own stream, outside the events
                case["backward_alone_resident_wall_ms"] = {"f2_cnn_input_gradient": lg, "torch_autograd": tg,
                                                           "ratio_torch_over_library_median": round(tg["median"] / lg["median"], 3)}
                for p in (d_x, d_g):
                    ctx.free(p)
                del xt
                torch.cuda.empty_cache()
            for name in ("host", "resident"):
                a1, b1, c1, a2, b2, c2 = timed(sal[name]), timed(occ[name]), timed(strided[name]), timed(sal[name]), timed(occ[name]), timed(strided[name])
                fa, oa, sa = stat(a1[0] + a2[0]), stat(b1[0] + b2[0]), stat(c1[0] + c2[0])
                case[name] = {"eval_saliency_batch_event_ms": fa, "eval_occlusion_batch_1to1_event_ms": oa, "eval_batch_strided_event_ms": sa,
                              "eval_saliency_batch_wall_ms": stat(a1[1] + a2[1]), "eval_occlusion_batch_1to1_wall_ms": stat(b1[1] + b2[1]),
                              "eval_batch_strided_wall_ms": stat(c1[1] + c2[1]),
                              "ratio_saliency_over_strided_median": round(fa["median"] / sa["median"], 3),
                              "ratio_occlusion_1to1_over_saliency_median": round(oa["median"] / fa["median"], 3),
                              "saliency_audio_s_per_s": round(B * n / FS / (fa["median"] * 1e-3), 1)}
            result["cases"].append(case)
            ctx.synchronize()
            for p in (d_wave, d_sc, d_lb, d_mp, d_sm, d_omp, d_osm):
                ctx.free(p)

if args.parent_lib and not args.only_strided:
    env = dict(os.environ, F2CNN_PROBE_LIB=os.path.abspath(args.parent_lib), F2CNN_PROBE_OLD_LIB="1")   # (a build without the newest entries loads)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-strided", "--utterances", args.utterances, "--samples", str(n),
                          "--hops", args.hops, "--reps", str(args.reps), "--warm", str(args.warm)], env=env, stdout=subprocess.PIPE, text=True,
                         timeout=900)
    if out.returncode == 0:
        parent = json.loads(out.stdout.strip().splitlines()[-1])["cases"]
        for case, p in zip(result["cases"], parent):
            for name in ("host", "resident"):
                ps = p[name]["eval_batch_strided_event_ms"]
                case[name]["parent_lib_eval_batch_strided_event_ms"] = ps
                case[name]["ratio_saliency_over_parent_strided_median"] = round(case[name]["eval_saliency_batch_event_ms"]["median"] / ps["median"], 3)
    else:
        result["parent_lib_error"] = out.returncode
if args.kernel_stats:
    result["chain_kernels"] = fold_kernel_stats(args.kernel_stats, args.kernel_stats_windows, args.kernel_stats_calls)

print(json.dumps(result), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result) + "\n")
ctx.close()
