"""Outputs of two builds of the library compared bit for bit (diagnostic; profiles/r08_a_old_new_identity.txt).
    python tools/old_new_identity.py run LIB OUT.json [KEEP_DIR] [--only=GROUP,...]    digests of every case's outputs with that
                                          library; with KEEP_DIR the outputs of the low-pass cases themselves are kept there (float64,
                                          ~1.3 GB); --only: the named groups alone (cnn_cases, entry_cases, sweep_cases, grad_cases,
                                          figure_cases, stage_cases, window_cases)
    python tools/old_new_identity.py compare OLD.json NEW.json [OLD_KEEP_DIR NEW_KEEP_DIR]    the table "case: identical /
                                          differs"; with the kept outputs, for a case that differs, the largest difference
                                          relative to the row maximum (envelopes: per utterance and channel; scores and windows:
                                          the whole array as one row)
Cases: f2_filterbank_envelope_fused, f2_eval_batch, f2_eval_utterance (one utterance) and f2_input_batch on single utterances of
1 700, 1 761, 16 000, 40 000 and 70 000 samples and on the 34-length ragged batch of tests/test_gpu_spectral.py; LPF off and
50 Hz; int16 waves, host memory, 128 channels. The CNN alone (profiles/r14_a_old_new_identity.txt): f2_cnn_forward on windows of
11 x 128, 11 x 67, 10 x 100 and 13 x 40 under the options float32 / per-tile split / ws convolutions / ws convolutions + ws dense1,
host and device memory, inputs in [0, 1), the same x 2^10, one window x 1e4 among normalised ones (the quiet-window route) and one
NaN, last_input_bound in the digest; one host call of 16 384 + 70 windows whose second chunk is x 2^6; f2_cnn_score_windows with
normalize 0 / 1 and three groups; the create-time *_check_diff values; f2_cnn_layers on the forced routes f32 and recorded for
13 x 40, 18 x 20, 14 x 24, 12 x 21 and 13 x 76 windows (pooled heights other than four, a second x-tile of the layer-by-layer kernels;
profiles/r40_a_old_new_identity.txt). The later entry points on small shapes
(profiles/r18_a_old_new_identity.txt; tests/test_gpu_output_placement.py: radius 5, step 160, utterances of 1761, 2500 and 1000
samples, an 11 x 10 network, 8 channels for the pictures), host and device memory, every output in the digest:
f2_eval_batch_strided at hop 1 and 160, f2_eval_noise_sweep with 2 levels and a fixed seed, f2_label_accuracy on its labels,
f2_envelope_picture / f2_gammatonegram_batch with both pools, f2_resample_batch at 3 : 2 and at the identity. The three sweeps
(profiles/r23_a_old_new_identity.txt): f2_eval_noise_sweep, f2_eval_cutoff_sweep and f2_eval_reverb_sweep with K = 2 on utterances
of 3000, 1000 (shorter than a window) and 2100 samples, int16 and float64, hop 16 and hop = STEP, host and device memory, the
optional outputs given and left out; levels, scores, labels, window offsets, sigma and stats in the digest. The backward pass and
the training step (profiles/r28_a_old_new_identity.txt), host and device memory, seeds fixed here: f2_cnn_input_gradient on an
11 x 10 network and 1024 + 70 windows (two chunks of the chain) and on 13 x 40 and 11 x 67 networks and 193 windows, all three
outputs and the scores alone; f2_cnn_layers on the recorded route; f2_cnn_loss_gradient on 1094 windows of 11 x 10 without and
with dropout, without an index and with a permutation that repeats, on 4100 windows from host memory (two host pieces), on none,
and on 193 windows of 13 x 40 - the 12 gradients, the loss sum and the hits in the digest; f2_trainer_steps twice over 70 windows
in batches of 32 - weights, accumulators, last gradient, loss, hits and iterations after each call; f2_eval_saliency_batch on the
case of tests/test_gpu_saliency_placement.py. The figure family (profiles/r37_a_old_new_identity.txt) on that case's utterances with
spans given, hop 16 and hop = STEP, host and device memory: f2_eval_figure_batch and f2_eval_occlusion_batch (K = 2 patches) with
every output, with each reduction alone and with none of them - every output given, window_offsets and the range in the digest;
f2_score_track, f2_occlusion_map and f2_saliency_map on random rows. The stage calls (profiles/r38_a_old_new_identity.txt):
f2_reverb_levels, f2_reverb_pick, f2_shaped_noise_levels, f2_noise_pick, f2_lowpass_levels and f2_channel_mix_levels on utterances
of 0, 1, 1023, 1024, 1025 and 3000 samples, int16 and float64, host and device memory, K = 3 with 1, 1025 and 2500 taps (rooms) and
2, 1025 and 2048 taps (noise filters), sigma given and left out, all-dry / all-clean stages and a batch without samples;
f2_input_batch_wet and a render_wet of the trainer with one pass of steps behind it; and per call the status and message of a
fixed list of invalid calls - those of tests/test_gpu_reverb_levels.py, tests/test_gpu_reverb_pick.py, tests/test_gpu_noise_pick.py
and ERROR_CASES of tests/test_gpu_shaped_noise.py, and calls with two things wrong at once (which one is named). The window calls with
augmentation stages (profiles/r42_a_old_new_identity.txt; radius 5, step 160, 8 channels, utterances of 1761, 2500 and 1000 samples,
int16 and float64, host and device memory): f2_input_batch_noisy / _wet / _coloured / _smeared with every stage active and with
each stage all-dry / all-clean / all-sharp in turn, f2_gather_windows_mixed; a trainer with group 2 over five utterances (10
channels) through render, render_wet, render(firs=) and render_wet(mixes=), the rendered windows and one pass of steps behind the
last; and per call the status and message of the invalid calls of the test_errors_* functions of
tests/test_gpu_input_batch_wet.py, _coloured.py, _smeared.py and tests/test_gpu_trainer_render.py, and one call per pair of adjacent
checks with both things wrong at once."""
import hashlib, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

C, RADIUS, STEP = 128, 5, 160
R = 2 * RADIUS + 1
RAGGED = [16000, 15999, 9000, 8193, 16320, 16321, 4097, 5000, 8128, 8129, 300, 16384, 20000, 1, 32704, 32705, 16385,
          27001, 40000, 32769, 65472, 65473, 50001, 65536, 33333, 70000, 16128, 16129, 7936, 7937, 32512, 32513, 65280, 65281]
BATCHES = [(f"one utterance of {n}", [n]) for n in (1700, 1761, 16000, 40000, 70000)] + [("ragged batch of 34", RAGGED)]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


CNN_SHAPES = [(11, 128), (11, 67), (10, 100), (13, 40)]
LAYER_SHAPES = [(13, 40), (18, 20), (14, 24), (12, 21), (13, 76)]
CNN_ROUTES = [("float32", 0, 0, 0), ("per-tile split", 1, 0, 0), ("ws convolutions", 1, 1, 0), ("ws convolutions + ws dense1", 1, 1, 1)]


def on_device(ctx, arrays, call):
    """call(*device pointers) with every array of `arrays` uploaded (None stays None); the arrays are read back afterwards"""
    ptrs = [None if a is None else ctx.malloc(max(a.nbytes, 4)) for a in arrays]
    try:
        for p, a in zip(ptrs, arrays):
            if p is not None:
                ctx.h2d(p, a)
        out = call(*ptrs)
        ctx.synchronize()
        for p, a in zip(ptrs, arrays):
            if p is not None:
                ctx.d2h(a, p)
    finally:
        for p in ptrs:
            if p is not None:
                ctx.free(p)
    return out


def cnn_cases(ctx, res):
    from f2cnn_amd import _lib
    from f2cnn_amd.model import F2CNNModel
    n = 193
    for rows, ch in CNN_SHAPES:
        m = F2CNNModel.glorot(7, rows, ch, zero_bias=False)
        h = m.handle(ctx)
        res[f"f2_cnn_create {rows} x {ch}: check diffs"] = digest(np.array(
            [ctx.cnn_info(h, k) for k in ("ws_ok", "ws_dense_ok", "f16x3_ok", "ws_check_diff", "ws_dense_check_diff", "f16x3_check_diff")]))
        x = np.random.default_rng(rows * ch).random((n, rows, ch)).astype(np.float32)
        spike, nan = x.copy(), x.copy()
        spike[5] *= 1e4
        nan[7, 2, 3] = np.nan
        signs = (np.arange(n) % 2).astype(np.uint8)
        groups = (np.arange(n) % 3).astype(np.int32)
        for rname, sp, ws, wsd in CNN_ROUTES:
            ctx.set_option("cnn_f16x3", sp)
            ctx.set_option("cnn_ws", ws)
            ctx.set_option("cnn_ws_dense", wsd)
            for mname, mem in (("host", _lib.MEM_HOST), ("device", _lib.MEM_DEVICE)):
                tag = f"{rows} x {ch}, {rname}, {mname} memory"
                for iname, xi in (("in [0, 1)", x), ("x 2^10", x * np.float32(1024)), ("one window x 1e4", spike), ("one NaN", nan)):
                    sc, lb = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
                    if mem == _lib.MEM_HOST:
                        ctx.cnn_forward(h, xi, n, sc, lb, mem)
                    else:
                        on_device(ctx, [np.ascontiguousarray(xi), sc, lb], lambda dx, ds, dl: ctx.cnn_forward(h, dx, n, ds, dl, mem))
                    res[f"f2_cnn_forward: {tag}, {iname}"] = digest(sc, lb, np.float64(ctx.cnn_info(h, "last_input_bound")))
                for norm in (0, 1):
                    w = x + np.float32(0.5)     # (strictly positive, as normalisation demands)
                    sc, lb = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
                    if mem == _lib.MEM_HOST:
                        counts, loss = ctx.cnn_score_windows(h, w, n, norm, signs, groups, 3, sc, lb, mem)
                    else:
                        counts, loss = on_device(ctx, [w, signs, groups, sc, lb], lambda dw, dsg, dg, ds, dl: ctx.cnn_score_windows(
                            h, dw, n, norm, dsg, dg, 3, ds, dl, mem))
                    res[f"f2_cnn_score_windows: {tag}, normalize {norm}"] = digest(sc, lb, counts, loss)
        for o in ("cnn_f16x3", "cnn_ws", "cnn_ws_dense"):
            ctx.set_option(o, 1)
        print(f"CNN {rows} x {ch} done", flush=True)
    m = F2CNNModel.glorot(7, 11, 40, zero_bias=False)
    x = np.random.default_rng(40).random((16384 + 70, 11, 40)).astype(np.float32)
    x[16384:] *= np.float32(64)
    sc, lb = np.zeros((len(x), 2), np.float32), np.zeros(len(x), np.uint8)
    ctx.cnn_forward(m.handle(ctx), x, len(x), sc, lb, _lib.MEM_HOST)
    res["f2_cnn_forward: 11 x 40, 16 384 + 70 windows in host memory, second chunk x 2^6"] = digest(
        sc, lb, np.float64(ctx.cnn_info(m.handle(ctx), "last_input_bound")))
    # the float32 kernels layer by layer (three, five, six and eight pooled rows; 13 x 76: a second x-tile) and the recorded forward
    for rows, ch in LAYER_SHAPES:
        m = F2CNNModel.glorot(7, rows, ch, zero_bias=False)
        x = np.random.default_rng(rows * ch + 1).random((33, rows, ch)).astype(np.float32)
        for route in ("f32", "recorded"):
            res[f"f2_cnn_layers: {rows} x {ch}, 33 windows, route {route}, host memory"] = digest(*m.layers(x, route, ctx=ctx))


def entry_cases(ctx, res):
    from f2cnn_amd import _lib
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.resample import design_resampler
    import f2cnn_oracle as orc
    lens, CN, CP, W = [1761, 2500, 1000], 10, 8, 7
    B = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(offs[-1])
    wave = np.concatenate([orc.synth_utterance(900 + i, n) for i, n in enumerate(lens)])
    coefs = {c: filters.make_erb_filters(16000, filters.centre_freqs(16000, c, 100)) for c in (CN, CP)}
    h = F2CNNModel.glorot(7, R, CN, zero_bias=False).handle(ctx)
    snr = np.array([20.0, 5.0])
    U = (len(snr) + 1) * B

    def both(name, inputs, outs, call):
        """call(mem, *inputs, *outs) in host memory and with every array on the device; host results of the call join the digest"""
        for mname, mem in (("host", _lib.MEM_HOST), ("device", _lib.MEM_DEVICE)):
            o = [np.zeros(n, dt) for dt, n in outs]
            extra = call(mem, *inputs, *o) if mem == _lib.MEM_HOST else on_device(ctx, list(inputs) + o, lambda *p: call(mem, *p))
            res[f"{name}, {mname} memory"] = digest(*o, *[np.asarray(e) for e in extra])
        return o

    for hop in (1, 160):
        n = sum(_lib.strided_window_count(x, RADIUS, STEP, hop) for x in lens)
        both(f"f2_eval_batch_strided: hop {hop}", [wave], [(np.float32, 2 * n), (np.uint8, n)], lambda mem, w, sc, lb: (
            ctx.eval_batch_strided(h, w, _lib.WAVE_I16, offs, coefs[CN], B, CN, True, 50.0, _lib.FFT_F32, RADIUS, STEP, hop, sc, lb, mem),))
    n = (len(snr) + 1) * sum(_lib.strided_window_count(x, RADIUS, STEP, 160) for x in lens)
    sweep = both("f2_eval_noise_sweep: 2 levels, seed 1234", [wave], [(np.float64, (len(snr) + 1) * total), (np.float32, 2 * n), (np.uint8, n)],
                 lambda mem, w, ny, sc, lb: ctx.eval_noise_sweep(h, w, _lib.WAVE_I16, offs, coefs[CN], B, CN, True, 50.0, _lib.FFT_F32, RADIUS, STEP,
                                                                  160, snr, 1234, ny, sc, lb, mem))
    wo = np.zeros(U + 1, np.int64)
    wo[1:] = np.cumsum([_lib.strided_window_count(x, RADIUS, STEP, 160) for x in lens] * (len(snr) + 1))
    both("f2_label_accuracy: the sweep's labels against three reference sets", [sweep[2]], [], lambda mem, lb: (ctx.label_accuracy(
        lb, wo, np.array([0, 1, 4, 5]), np.array([900, 850, 1200, 2000, 400]), np.array([1, 0, 1, 0, 1]), RADIUS * STEP, 160, STEP, mem),))
    env = np.zeros(CP * total)
    ctx.filterbank_envelope_fused(wave, _lib.WAVE_I16, offs, coefs[CP], B, CP, True, 50.0, _lib.FFT_F32, env, None, _lib.MEM_HOST)
    pix = [(np.float64, B * CP * W), (np.uint8, B * CP * W)]
    for pool in (0, 1):
        both(f"f2_envelope_picture: width {W}, pool {pool}", [env], pix, lambda mem, e, po, lv: (
            ctx.envelope_picture(e, offs, B, CP, None, W, pool, po, lv, mem),))
        both(f"f2_gammatonegram_batch: width {W}, pool {pool}", [wave], pix, lambda mem, w, po, lv: (
            ctx.gammatonegram_batch(w, _lib.WAVE_I16, offs, coefs[CP], B, CP, True, 50.0, _lib.FFT_F32, None, W, pool, po, lv, mem),))
    audio = np.random.default_rng(8).integers(-20000, 20000, (300, 2)).astype(np.int16)
    for up, down in ((3, 2), (1, 1)):
        _, _, half_len, taps = design_resampler(down, up)
        both(f"f2_resample_batch: {up} : {down}, int16 stereo, 300 frames", [audio], [(np.float64, _lib.resampled_length(300, up, down))],
             lambda mem, a, out: (ctx.resample_batch(a, _lib.PCM_I16, 2, -1, np.array([0, 300]), 1, up, down, taps, half_len, out, mem),))
    print("later entry points done", flush=True)


def sweep_cases(ctx, res):
    from f2cnn_amd import _lib
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel
    import f2cnn_oracle as orc
    lens, CN, K = [3000, 1000, 2100], 10, 2
    B = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(offs[-1])
    i16 = np.concatenate([orc.synth_utterance(700 + i, n) for i, n in enumerate(lens)])
    coefs = filters.make_erb_filters(16000, filters.centre_freqs(16000, CN, 100))
    h = F2CNNModel.glorot(7, R, CN, zero_bias=False).handle(ctx)
    rng = np.random.default_rng(23)
    rirs = [np.concatenate([[1.0], 0.1 * rng.standard_normal(n - 1) * np.exp(-np.arange(1, n) / (n / 7.0))]) for n in (300, 1500)]
    tail = (coefs, B, CN, True, 50.0, _lib.FFT_F32, RADIUS, STEP)
    sweeps = [     # name, doubles of a level per sample, the call
        ("f2_eval_noise_sweep", 1, lambda w, dt, hop, lv, sc, lb, mem: ctx.eval_noise_sweep(
            h, w, dt, offs, *tail, hop, np.array([20.0, 5.0]), 1234, lv, sc, lb, mem)),
        ("f2_eval_cutoff_sweep", CN, lambda w, dt, hop, lv, sc, lb, mem: ctx.eval_cutoff_sweep(
            h, w, dt, offs, coefs, B, CN, _lib.FFT_F32, RADIUS, STEP, hop, np.array([8.0, 50.0]), lv, sc, lb, mem)),
        ("f2_eval_reverb_sweep", 1, lambda w, dt, hop, lv, sc, lb, mem: ctx.eval_reverb_sweep(h, w, dt, offs, *tail, hop, rirs, lv, sc, lb, mem)),
    ]
    for dname, dt, wave in (("int16", _lib.WAVE_I16, i16), ("float64", _lib.WAVE_F64, i16.astype(np.float64))):
        for hop in (16, STEP):
            n = (K + 1) * sum(_lib.strided_window_count(x, RADIUS, STEP, hop) for x in lens)
            for name, per, call in sweeps:
                for mname, mem in (("host", _lib.MEM_HOST), ("device", _lib.MEM_DEVICE)):
                    for given in (True, False):
                        o = [np.zeros((K + 1) * per * total), np.zeros(2 * n, np.float32), np.zeros(n, np.uint8)] if given else [None] * 3
                        small = call(wave, dt, hop, *o, mem) if mem == _lib.MEM_HOST else on_device(
                            ctx, [wave] + o, lambda w, lv, sc, lb: call(w, dt, hop, lv, sc, lb, mem))
                        res[f"{name}: {dname}, hop {hop}, {mname} memory, optional outputs {'given' if given else 'left out'}"] = digest(
                            *[a for a in o if a is not None], *[np.asarray(a) for a in small])
    print("sweeps done", flush=True)


def grad_cases(ctx, res):
    from f2cnn_amd import _lib
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel, tensor_shapes
    from f2cnn_amd.trainer import Trainer
    import f2cnn_oracle as orc
    MEMS = (("host", _lib.MEM_HOST), ("device", _lib.MEM_DEVICE))
    DROP = (0.25, 0.25, 0.5)

    def windows(seed, n, rows, ch):
        rng = np.random.default_rng(seed)
        return rng.random((n, rows, ch)).astype(np.float32), rng.integers(0, 2, n).astype(np.uint8)

    # f2_cnn_input_gradient: 1024 + 70 windows cross the chain's chunk; 13 x 40 has an odd row count after conv2, 11 x 67 an odd width
    for rows, ch, n in ((R, 10, 1094), (13, 40, 193), (R, 67, 193)):
        h = F2CNNModel.glorot(7, rows, ch, zero_bias=False).handle(ctx)
        x, _ = windows(rows * ch + n, n, rows, ch)
        for mname, mem in MEMS:
            for oname, full in (("gradient, profile and scores", True), ("scores alone", False)):
                G, prof, sc = np.zeros((n, rows, ch), np.float32), np.zeros((n, ch, 2)), np.zeros((n, 2), np.float32)
                outs = [G, prof, sc] if full else [None, None, sc]
                if mem == _lib.MEM_HOST:
                    ctx.cnn_input_gradient(h, x, n, *outs, mem)
                else:
                    on_device(ctx, [x] + outs, lambda dx, dg, dp, ds: ctx.cnn_input_gradient(h, dx, n, dg, dp, ds, mem))
                res[f"f2_cnn_input_gradient: {rows} x {ch}, {n} windows, {oname}, {mname} memory"] = digest(*[a for a in outs if a is not None])
    small = F2CNNModel.glorot(7, R, 10, zero_bias=False)
    h = small.handle(ctx)
    flat = tensor_shapes(R, 10)["dense1_w"][0]
    x, _ = windows(193, 193, R, 10)
    for mname, mem in MEMS:
        outs = [np.zeros((193, flat), np.float32), np.zeros((193, 516), np.float32), np.zeros((193, 2), np.float32)]
        if mem == _lib.MEM_HOST:
            ctx.cnn_layers(h, x, 193, _lib.CNN_ROUTES["recorded"], *outs, mem)
        else:
            on_device(ctx, [x] + outs, lambda dx, dp, d1, ds: ctx.cnn_layers(h, dx, 193, _lib.CNN_ROUTES["recorded"], dp, d1, ds, mem))
        res[f"f2_cnn_layers: recorded route, {R} x 10, 193 windows, {mname} memory"] = digest(*outs)
    print("input gradient done", flush=True)

    def loss_gradient(name, model, x, y, index, m, drop, mems=MEMS):
        shapes = list(tensor_shapes(model.rows, model.channels).values())
        hm = model.handle(ctx)
        for mname, mem in mems:
            grads = [np.full(s, 7.0, np.float32) for s in shapes]
            if mem == _lib.MEM_HOST:
                loss, hits = ctx.cnn_loss_gradient(hm, x, y, index, m, drop, 99, 3, grads, mem)
            else:
                loss, hits = on_device(ctx, [x, y, index] + grads, lambda dx, dy, di, *dg: ctx.cnn_loss_gradient(
                    hm, dx, dy, di, m, drop, 99, 3, list(dg), mem))
            res[f"f2_cnn_loss_gradient: {name}, {mname} memory"] = digest(*grads, np.float64(loss), np.int64(hits))

    n = 1094
    x, y = windows(11, n, R, 10)
    index = np.random.default_rng(12).permutation(n).astype(np.int64)
    index[5::97] = index[3]                                   # (repeats)
    for drop in ((0.0, 0.0, 0.0), DROP):
        for iname, idx in (("no index", None), ("index a permutation with repeats", index)):
            loss_gradient(f"{R} x 10, {n} windows, dropout {drop}, {iname}", small, x, y, idx, n, drop)
    loss_gradient(f"{R} x 10, m = 0", small, x[:1], y[:1], None, 0, DROP)
    xl, yl = windows(13, 4100, R, 10)
    loss_gradient(f"{R} x 10, 4100 windows (two host pieces), dropout {DROP}", small, xl, yl, None, 4100, DROP, MEMS[:1])
    x, y = windows(14, 193, 13, 40)
    loss_gradient(f"13 x 40, 193 windows, dropout {DROP}", F2CNNModel.glorot(7, 13, 40, zero_bias=False), x, y, None, 193, DROP)
    print("loss gradient done", flush=True)

    # f2_trainer_steps: 70 windows in batches of 32 (the last one of 6), twice
    x, y = windows(15, 70, R, 10)
    tr = Trainer(small, lr=1e-3, decay=1e-6, drop=DROP, seed=5, ctx=ctx)
    tr.set_data(x, y)
    for call in (1, 2):
        loss, hits = tr.steps(np.random.default_rng(15 + call).permutation(70), 32)
        res[f"f2_trainer_steps: {R} x 10, 70 windows, batch 32, call {call}"] = digest(
            *tr.weights().values(), *tr.accumulators().values(), *tr.gradient().values(), np.float64(loss), np.int64(hits), np.int64(tr.iterations))
    tr.close()

    # f2_eval_saliency_batch: the case of tests/test_gpu_saliency_placement.py
    lens, CS, W, hop = [2500, 1761, 3001, 1700], 16, 40, 16
    B = len(lens)
    coefs = np.ascontiguousarray(filters.make_erb_filters(16000, filters.centre_freqs(16000, CS, 100)))
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wave = np.concatenate([orc.synth_utterance(3100 + i, k) for i, k in enumerate(lens)]).astype(np.int16)
    nwin = sum(_lib.strided_window_count(k, RADIUS, STEP, hop) for k in lens)
    h = F2CNNModel.glorot(7, R, CS, zero_bias=False).handle(ctx)
    for mname, mem in MEMS:
        outs = [np.zeros((B, CS, W), np.uint8), np.zeros((B, CS, W, 3)), np.zeros((B, CS, 3)), np.zeros((nwin, 2), np.float32),
                np.zeros(nwin, np.uint8)]
        call = lambda w, lv, mp, sm, sc, lb: ctx.eval_saliency_batch(h, w, _lib.WAVE_I16, offs, coefs, B, CS, True, 50.0, _lib.FFT_F32, RADIUS, STEP,
                                                                    hop, None, W, 0, lv, mp, sm, sc, lb, mem)
        wo, rng = call(wave, *outs) if mem == _lib.MEM_HOST else on_device(ctx, [wave] + outs, call)
        res[f"f2_eval_saliency_batch: 4 utterances, 16 channels, hop 16, {mname} memory"] = digest(*outs, wo, rng)
    print("gradient cases done", flush=True)


def figure_cases(ctx, res):
    from f2cnn_amd import _lib
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel
    import f2cnn_oracle as orc
    MEMS = (("host", _lib.MEM_HOST), ("device", _lib.MEM_DEVICE))
    lens, CS, W, K = [2500, 1761, 3001, 1700], 16, 40, 2       # (the saliency case of grad_cases; 1700 is shorter than a window)
    B = len(lens)
    coefs = np.ascontiguousarray(filters.make_erb_filters(16000, filters.centre_freqs(16000, CS, 100)))
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    wave = np.concatenate([orc.synth_utterance(3100 + i, k) for i, k in enumerate(lens)]).astype(np.int16)
    spans = np.array([[100, 2400], [0, 1761], [500, 3001], [0, 1700]], np.int64)
    patches, fillv = np.array([[0, R, 0, 8], [3, 8, 4, CS]], np.int32), 0.25
    h = F2CNNModel.glorot(7, R, CS, zero_bias=False).handle(ctx)
    for hop in (16, STEP):
        front = (_lib.WAVE_I16, offs, coefs, B, CS, True, 50.0, _lib.FFT_F32, RADIUS, STEP, hop)
        wo = np.concatenate([[0], np.cumsum([_lib.strided_window_count(k, RADIUS, STEP, hop) for k in lens])]).astype(np.int64)
        n = int(wo[-1])
        fused = [
            ("f2_eval_figure_batch", dict(levels=((B, CS, W), np.uint8), track=((B, W, 5), np.float64), scores=((n, 2), np.float32), labels=(n, np.uint8)),
             lambda mem, w, lv, tr, sc, lb: ctx.eval_figure_batch(h, w, *front, spans, W, 0, lv, tr, sc, lb, mem),
             (("every output", "levels track scores labels"), ("the track alone", "track"), ("no track", "levels scores labels"))),
            ("f2_eval_occlusion_batch", dict(levels=((B, CS, W), np.uint8), map=((B, K, W, 4), np.float64), summary=((B, K, 4), np.float64),
                                             scores=((n, K + 1, 2), np.float32), labels=((n, K + 1), np.uint8)),
             lambda mem, w, lv, mp, sm, sc, lb: ctx.eval_occlusion_batch(h, w, *front, patches, fillv, spans, W, 0, lv, mp, sm, sc, lb, mem),
             (("every output", "levels map summary scores labels"), ("the map alone", "map"), ("the summary alone", "summary"),
              ("neither map nor summary", "levels scores labels"))),
        ]
        for name, shapes, call, variants in fused:
            for mname, mem in MEMS:
                for vname, given in variants:
                    outs = [np.zeros(s, dt) if k in given.split() else None for k, (s, dt) in shapes.items()]
                    f = lambda *p: call(mem, *p)
                    small = f(wave, *outs) if mem == _lib.MEM_HOST else on_device(ctx, [wave] + outs, f)
                    res[f"{name}: hop {hop}, {mname} memory, {vname}"] = digest(*[a for a in outs if a is not None], *small)
        # the reductions alone, on rows that do not come from the library
        rng = np.random.default_rng(370 + hop)
        sc = rng.standard_normal((n, K + 1, 2)).astype(np.float32)
        lb = (sc[..., 1] > sc[..., 0]).astype(np.uint8)
        prof, origin = rng.standard_normal((n, CS, 2)), RADIUS * STEP
        alone = [
            ("f2_score_track", [sc[:, 0].copy(), lb[:, 0].copy()], (B, W, 5), lambda mem, s, l, o: ctx.score_track(s, l, wo, spans, origin, hop, W, o, mem)),
            ("f2_occlusion_map", [sc, lb], (B, K, W, 4), lambda mem, s, l, o: ctx.occlusion_map(s, l, wo, K, spans, origin, hop, W, o, mem)),
            ("f2_saliency_map", [prof], (B, CS, W, 3), lambda mem, p, o: ctx.saliency_map(p, wo, CS, spans, origin, hop, W, o, mem)),
        ]
        for name, ins, shape, call in alone:
            for mname, mem in MEMS:
                out = np.zeros(shape)
                if mem == _lib.MEM_HOST:
                    call(mem, *ins, out)
                else:
                    on_device(ctx, ins + [out], lambda *p: call(mem, *p))
                res[f"{name}: hop {hop}, {mname} memory"] = digest(out)
    print("figure cases done", flush=True)


def stage_cases(ctx, res):
    """the six stage calls (profiles/r38_a_old_new_identity.txt): outputs, sigma given and left out, and the status and message
    of the invalid calls of tests/test_gpu_reverb_levels.py, test_gpu_reverb_pick.py, test_gpu_noise_pick.py (their CASES) and
    tests/test_gpu_shaped_noise.py (ERROR_CASES)"""
    from f2cnn_amd import _lib
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.trainer import Trainer
    MEMS = (("host", _lib.MEM_HOST), ("device", _lib.MEM_DEVICE))
    INV, UNS = _lib.F2_ERR_INVALID, _lib.F2_ERR_UNSUPPORTED
    lens, K, CE = [0, 1, 1023, 1024, 1025, 3000], 3, 10
    B = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(offs[-1])
    rng = np.random.default_rng(38)
    i16 = rng.integers(-20000, 20000, total).astype(np.int16)
    rirs = [rng.standard_normal(t) * np.exp(-np.arange(t) / (t / 5.0 + 1)) for t in (1, 1025, 2500)]
    firs = [h / np.sqrt(h @ h) for h in (rng.standard_normal(t) for t in (2, 1025, 2048))]
    snr, seed = np.array([10.0, -3.0, 20.0]), 0x1234_5678_9ABC
    ftaps, foffs = _lib._pack_firs(firs, K)
    room_of, level_of = np.arange(B, dtype=np.int32) % (K + 1), (np.arange(B, dtype=np.int32) + 1) % (K + 1)
    env = np.abs(rng.standard_normal(CE * total)) + 0.01
    mix = rng.standard_normal((K, CE, CE)) * (np.abs(np.subtract.outer(np.arange(CE), np.arange(CE))) < 3)
    cutoffs = np.array([8.0, 50.0, 400.0])

    def both(name, inputs, outs, call):
        for mname, mem in MEMS:
            o = [np.zeros(n, dt) for dt, n in outs]
            extra = call(mem, *inputs, *o) if mem == _lib.MEM_HOST else on_device(ctx, list(inputs) + o, lambda *p: call(mem, *p))
            res[f"{name}, {mname} memory"] = digest(*o, *[np.asarray(e) for e in extra if e is not None])

    for dname, dt, wave in (("int16", _lib.WAVE_I16, i16), ("float64", _lib.WAVE_F64, i16.astype(np.float64))):
        both(f"f2_reverb_levels: {dname}", [wave], [(np.float64, (K + 1) * total)],
             lambda mem, w, o: (ctx.reverb_levels(w, dt, offs, B, rirs, o, mem),))
        both(f"f2_reverb_pick: {dname}", [wave], [(np.float64, total)], lambda mem, w, o: (ctx.reverb_pick(w, dt, offs, B, rirs, room_of, o, mem),))
        both(f"f2_reverb_pick: {dname}, every utterance dry", [wave], [(np.float64, total)],
             lambda mem, w, o: (ctx.reverb_pick(w, dt, offs, B, rirs, None, o, mem),))
        both(f"f2_shaped_noise_levels: {dname}, sigma given", [wave], [(np.float64, (K + 1) * total)],
             lambda mem, w, o: (ctx.shaped_noise_levels(w, dt, offs, B, snr, firs, seed, o, mem),))
        both(f"f2_shaped_noise_levels: {dname}, sigma left out", [wave], [(np.float64, (K + 1) * total)], lambda mem, w, o: (
            ctx.check(ctx.lib.f2_shaped_noise_levels(ctx.handle, _lib._ptr(w), dt, offs.ctypes.data, B, snr.ctypes.data, ftaps.ctypes.data,
                                                     foffs.ctypes.data, K, seed, _lib._ptr(o), None, mem)),))
        for sname, sg in (("given", True), ("left out", None)):
            both(f"f2_noise_pick: {dname}, sigma {sname}", [wave], [(np.float64, total)],
                 lambda mem, w, o: (ctx.noise_pick(w, dt, offs, B, snr, level_of, 7, seed, o, mem, sigma=sg),))
            both(f"f2_noise_pick: {dname}, every utterance clean, sigma {sname}", [wave], [(np.float64, total)],
                 lambda mem, w, o: (ctx.noise_pick(w, dt, offs, B, snr, None, 7, seed, o, mem, sigma=sg),))
    both("f2_lowpass_levels", [env], [(np.float64, (K + 1) * CE * total)], lambda mem, e, o: (ctx.lowpass_levels(e, offs, B, CE, cutoffs, o, mem),))
    both("f2_channel_mix_levels", [env], [(np.float64, (K + 1) * CE * total)], lambda mem, e, o: (ctx.channel_mix_levels(e, offs, B, CE, mix, o, mem),))
    # empty batches: nothing written, sigma zeroed
    zeros5, sig = np.zeros(B + 1, np.int64), np.full((K + 1) * B, 7.0)
    ctx.shaped_noise_levels(None, _lib.WAVE_I16, zeros5, B, snr, firs, seed, None, _lib.MEM_HOST, sigma=sig)
    sig2 = ctx.noise_pick(None, _lib.WAVE_I16, zeros5, B, snr, level_of, 0, seed, None, _lib.MEM_HOST, sigma=np.full(B, 7.0))
    res["f2_shaped_noise_levels / f2_noise_pick: utterances without samples, sigma"] = digest(sig, sig2)
    print("stage outputs done", flush=True)

    # f2_input_batch_wet and a render_wet of the trainer on the utterances long enough for a window
    wl = [3000, 2500, 1761]
    woffs = np.concatenate([[0], np.cumsum(wl)]).astype(np.int64)
    ww = rng.integers(-20000, 20000, int(woffs[-1])).astype(np.int16)
    coefs = np.ascontiguousarray(filters.make_erb_filters(16000, filters.centre_freqs(16000, CE, 100)))
    cs = [np.array([RADIUS * STEP, n - 1 - RADIUS * STEP], np.int64) for n in wl]
    coffs = np.arange(0, 2 * len(wl) + 1, 2, dtype=np.int64)
    rooms, levs = np.array([0, 3, 2], np.int32), np.array([1, 0, 3], np.int32)
    both("f2_input_batch_wet: three utterances, K = 3 rooms, 3 noise levels", [ww], [(np.float32, 2 * len(wl) * R * CE)], lambda mem, w, o: (
        ctx.input_batch_wet(w, _lib.WAVE_I16, woffs, coefs, len(wl), CE, True, 50.0, _lib.FFT_F32, coffs, np.concatenate(cs), RADIUS, STEP, True,
                            rirs, rooms, snr, levs, 0, seed, o, mem),))
    tr = Trainer(F2CNNModel.glorot(7, R, CE, zero_bias=False), lr=1e-3, decay=1e-6, drop=(0.0, 0.0, 0.0), seed=5, ctx=ctx)
    tr.set_waves([ww[a:b] for a, b in zip(woffs[:-1], woffs[1:])], cs, [np.array([0, 1], np.uint8)] * len(wl), coefs, RADIUS, STEP, lpf=True)
    tr.render_wet(rirs=rirs, room_of=rooms, snrs=snr, level_of=levs, seed=seed)
    res["f2_trainer_render_wet: three utterances, the rendered windows"] = digest(*tr.windows())
    tr.close()
    print("wet windows done", flush=True)

    # invalid calls: status and message
    p = lambda a: None if a is None else a.ctypes.data
    eo = np.array([0, 65, 67, 130], np.int64)
    ew = np.arange(130).astype(np.int16)
    bad0, dec = eo.copy(), eo.copy()
    bad0[0], dec[2] = 1, dec[1] - 1
    tap = {"rir": np.array([1.0, 0.5, 0.25, 1.0]), "ro": np.array([0, 3, 4], np.int64), "k": 2}
    nan, inf = tap["rir"].copy(), tap["rir"].copy()
    nan[3], inf[3] = np.nan, -np.inf
    table_cases = [("K=65", dict(rir=np.ones(65), ro=np.arange(66, dtype=np.int64), k=65)), ("rir NULL", dict(rir=None)),
                   ("rir_offsets NULL", dict(ro=None)), ("rir_offsets[0]=1", dict(ro=np.array([1, 3, 4], np.int64))),
                   ("rir_offsets decreasing", dict(ro=np.array([0, 3, 2], np.int64))), ("no taps", dict(ro=np.array([0, 4, 4], np.int64))),
                   ("tap nan", dict(rir=nan)), ("tap inf", dict(rir=inf)),
                   ("32769 taps", dict(rir=np.full(32770, 1e-3), ro=np.array([0, 1, 32770], np.int64)))]
    batch_cases = [("B<0", dict(nb=-1)), ("wave_dtype", dict(dt=2)), ("offsets NULL", dict(off=None)), ("offsets[0]=1", dict(off=bad0)),
                   ("offsets decreasing", dict(off=dec)), ("wave NULL", dict(wave=None)), ("output NULL", dict(out=None)), ("mem_space", dict(mem=7)),
                   # two things wrong at once: which one the call names
                   ("B<0 and wave_dtype", dict(nb=-1, dt=2)), ("wave_dtype and mem_space", dict(dt=2, mem=7)),
                   ("offsets decreasing and the call's own check", dict(off=dec, k=-1))]
    out = np.zeros(3 * 130)

    def invalid(name, call, cases):
        rows = []
        for cname, kw in cases:
            rc = call(**kw)
            rows.append(f"{cname}: {rc} {ctx.lib.f2_last_error(ctx.handle).decode()}")
            assert rc != _lib.F2_OK, (name, cname)
        res[f"{name}: {len(cases)} invalid calls, status and message"] = digest(np.frombuffer("\n".join(rows).encode(), np.uint8))

    def levels_call(wave=ew, dt=_lib.WAVE_I16, off=eo, nb=3, rir=tap["rir"], ro=tap["ro"], k=2, out=out, mem=_lib.MEM_HOST):
        return ctx.lib.f2_reverb_levels(ctx.handle, p(wave), dt, p(off), nb, p(rir), p(ro), k, p(out), mem)
    big = 1 << 24
    invalid("f2_reverb_levels", levels_call, [("K=0", dict(k=0))] + table_cases + [("levels x utterances", dict(
        nb=big, off=np.zeros(big + 1, np.int64), rir=np.ones(64), ro=np.arange(65, dtype=np.int64), k=64))] + batch_cases)

    room = np.array([0, 2, 1], np.int32)
    r3, rm1 = room.copy(), room.copy()
    r3[1], rm1[1] = 3, -1

    def pick_call(wave=ew, dt=_lib.WAVE_I16, off=eo, nb=3, rir=tap["rir"], ro=tap["ro"], k=2, room=room, out=out, mem=_lib.MEM_HOST):
        return ctx.lib.f2_reverb_pick(ctx.handle, p(wave), dt, p(off), nb, p(rir), p(ro), k, p(room), p(out), mem)
    invalid("f2_reverb_pick", pick_call, [("K<0", dict(k=-1)), ("room 3", dict(room=r3)), ("room -1", dict(room=rm1))] + table_cases + batch_cases)

    lev = np.array([0, 2, 1], np.int32)
    high, neg = lev.copy(), lev.copy()
    high[2], neg[1] = K + 1, -1
    nsnr, isnr = snr.copy(), snr.copy()
    nsnr[1], isnr[0] = np.nan, np.inf
    sigma = np.zeros(4 * 3)

    def noise_call(wave=ew, dt=_lib.WAVE_I16, off=eo, nb=3, s=snr, k=K, lv=lev, first=0, out=out, mem=_lib.MEM_HOST):
        return ctx.lib.f2_noise_pick(ctx.handle, p(wave), dt, p(off), nb, p(s), k, p(lv), first, seed, p(out), p(sigma), mem)
    invalid("f2_noise_pick", noise_call, [
        ("wave_dtype", dict(dt=7)), ("mem_space", dict(mem=5)), ("mem_space async", dict(mem=_lib.MEM_HOST_ASYNC)), ("offsets NULL", dict(off=None)),
        ("offsets[0]=1", dict(off=bad0)), ("offsets decreasing", dict(off=dec)), ("B<0", dict(nb=-1)), ("snr nan", dict(s=nsnr)),
        ("snr inf", dict(s=isnr)), ("K<0", dict(k=-1)), ("snr NULL", dict(s=None)), ("level high", dict(lv=high)), ("level negative", dict(lv=neg)),
        ("levels x utterances", dict(k=2 ** 30)), ("utterance number", dict(first=2 ** 32 - 3 + 1)), ("wave NULL", dict(wave=None)),
        ("output NULL", dict(out=None)), ("B<0 and wave_dtype", dict(nb=-1, dt=7)), ("B<0 and mem_space", dict(nb=-1, mem=5)),
        ("offsets decreasing and level high", dict(off=dec, lv=high)), ("offsets NULL and K<0", dict(off=None, k=-1))])

    f3 = [np.ones(1), np.ones(3) / np.sqrt(3), np.ones(2) / np.sqrt(2)]
    fir, fo = _lib._pack_rirs(f3)
    finf = fir.copy()
    finf[2] = np.inf
    many = _lib._pack_rirs([np.ones(1), np.ones(2049) / np.sqrt(2049), np.ones(2)])
    k65 = _lib._pack_rirs([np.ones(1)] * 65)

    def shaped_call(wave=ew, dt=_lib.WAVE_I16, off=eo, nb=3, s=snr, fir=fir, fo=fo, k=K, out=np.zeros(4 * 130), mem=_lib.MEM_HOST):
        return ctx.lib.f2_shaped_noise_levels(ctx.handle, p(wave), dt, p(off), nb, p(s), p(fir), p(fo), k, seed, p(out), p(sigma), mem)
    invalid("f2_shaped_noise_levels", shaped_call, [
        ("K=0", dict(k=0)), ("snr NULL", dict(s=None)), ("snr nan", dict(s=nsnr)), ("offsets decreasing", dict(off=dec)), ("fir NULL", dict(fir=None)),
        ("fir_offsets NULL", dict(fo=None)), ("fir_offsets[0] != 0", dict(fo=fo + 1, fir=np.concatenate([[0.5], fir]))),
        ("fir_offsets decreasing", dict(fo=np.array([0, 4, 3, 6], np.int64))), ("a level with no taps", dict(fo=np.array([0, 1, 6, 6], np.int64))),
        ("a tap that is not finite", dict(fir=finf)), ("too many taps", dict(fir=many[0], fo=many[1])),
        ("K=65", dict(k=65, s=np.zeros(65), fir=k65[0], fo=k65[1]))] + [c for c in batch_cases if "own check" not in c[0]] + [
        ("offsets decreasing and snr nan", dict(off=dec, s=nsnr))])

    def env_call(f):
        return lambda env=env[:CE * 130], off=eo, nb=3, c=CE, k=K, out=np.zeros(4 * CE * 130), mem=_lib.MEM_HOST, **kw: f(env, off, nb, c, k, out, mem, **kw)
    env_cases = [("B<0", dict(nb=-1)), ("C=0", dict(c=0)), ("mem_space", dict(mem=7)), ("mem_space async", dict(mem=_lib.MEM_HOST_ASYNC)),
                 ("offsets NULL", dict(off=None)), ("offsets decreasing", dict(off=dec)), ("K=0", dict(k=0)), ("K=65", dict(k=65)),
                 ("env NULL", dict(env=None)), ("output NULL", dict(out=None)), ("offsets decreasing and K=0", dict(off=dec, k=0))]
    invalid("f2_lowpass_levels", env_call(lambda e, off, nb, c, k, o, mem, cut=np.resize(cutoffs, 65): ctx.lib.f2_lowpass_levels(
        ctx.handle, p(e), p(off), nb, c, p(cut), k, p(o), mem)), env_cases + [("cutoff 9000 Hz", dict(cut=np.array([8.0, 9000.0, 50.0]))), ("cutoffs NULL", dict(cut=None))])
    invalid("f2_channel_mix_levels", env_call(lambda e, off, nb, c, k, o, mem, m=np.resize(mix, (65, CE, CE)): ctx.lib.f2_channel_mix_levels(
        ctx.handle, p(e), p(off), nb, c, p(m), k, p(o), mem)), env_cases + [("weight nan", dict(m=np.full((K, CE, CE), np.nan))), ("mix NULL", dict(m=None)),
                                                                          ("C=513", dict(c=513))])
    print("stage cases done", flush=True)


def window_cases(ctx, res):
    """the window calls with augmentation stages and the trainer's renders (profiles/r42_a_old_new_identity.txt): outputs with every
    stage active and with each stage idle in turn, the renders of a trainer in groups with one pass of steps behind the last, and
    the status and message of invalid calls - those of the test_errors_* functions of tests/test_gpu_input_batch_wet.py,
    test_gpu_input_batch_coloured.py, test_gpu_input_batch_smeared.py and test_gpu_trainer_render.py, and one call per pair of
    adjacent checks with both things wrong at once"""
    from f2cnn_amd import _lib
    from f2cnn_amd.gammatone import filters
    from f2cnn_amd.model import F2CNNModel
    from f2cnn_amd.trainer import Trainer
    import f2cnn_oracle as orc
    MEMS = (("host", _lib.MEM_HOST), ("device", _lib.MEM_DEVICE))
    INV = _lib.F2_ERR_INVALID
    lens, CW, CT = [1761, 2500, 1000], 8, 10       # (1000 samples: no room for a window; an 11 x 8 network has no dense1 input, so
    B = len(lens)                                  # the trainer renders 10 channels)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    i16 = np.concatenate([orc.synth_utterance(4200 + i, n) for i, n in enumerate(lens)]).astype(np.int16)
    coefs = {c: np.ascontiguousarray(filters.make_erb_filters(16000, filters.centre_freqs(16000, c, 100))) for c in (CW, CT)}
    reach = RADIUS * STEP
    cs = [np.array([reach, n // 2, n - 1 - reach], np.int64) if n > 2 * reach else np.zeros(0, np.int64) for n in lens]
    cen, coffs = np.concatenate(cs), np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    n = int(coffs[-1])
    rng = np.random.default_rng(42)
    rirs = [rng.standard_normal(t) * np.exp(-np.arange(t) / (t / 5.0 + 1)) for t in (7, 1025)]
    firs = [h / np.sqrt(h @ h) for h in (rng.standard_normal(t) for t in (5, 1025))]
    snr, seed, first = np.array([20.0, 3.0]), 0x1234_5678_9ABC, 7
    KR, K, KM = len(rirs), len(snr), 3

    def mixes(c):
        return rng.random((KM, c, c)) * (np.abs(np.subtract.outer(np.arange(c), np.arange(c))) < 3)   # (weights >= 0: the windows are normalised)
    mix = mixes(CW)
    room_of, level_of, mix_of = np.array([1, 2, 0], np.int32), np.array([0, 2, 1], np.int32), np.array([1, 3, 0], np.int32)
    idle = {"all dry": dict(room_of=np.full(B, KR, np.int32)), "all clean": dict(level_of=np.full(B, K, np.int32)),
            "all sharp": dict(mix_of=np.full(B, KM, np.int32))}
    entries = {     # the stages an entry has, and its call
        "noisy": ("all clean",), "wet": ("all dry", "all clean"), "coloured": ("all dry", "all clean"),
        "smeared": ("all dry", "all clean", "all sharp")}

    def stage_args(entry, room_of=room_of, level_of=level_of, mix_of=mix_of):
        return {"noisy": (snr, level_of, first, seed), "wet": (rirs, room_of, snr, level_of, first, seed),
                "coloured": (rirs, room_of, snr, firs, level_of, first, seed),
                "smeared": (rirs, room_of, snr, firs, level_of, first, seed, mix, mix_of)}[entry]

    def both(name, inp, size, call):
        for mname, mem in MEMS:
            o = np.zeros(size, np.float32)
            if mem == _lib.MEM_HOST:
                call(mem, inp, o)
            else:
                on_device(ctx, [inp, o], lambda di, do: call(mem, di, do))
            res[f"{name}, {mname} memory"] = digest(o)

    for dname, dt, wave in (("int16", _lib.WAVE_I16, i16), ("float64", _lib.WAVE_F64, i16.astype(np.float64) * 0.37)):
        for entry, idles in entries.items():
            for vname in ("every stage active",) + idles:
                args = stage_args(entry, **idle.get(vname, {}))
                both(f"f2_input_batch_{entry}: {dname}, {vname}", wave, n * R * CW, lambda mem, w, o: getattr(ctx, "input_batch_" + entry)(
                    w, dt, offs, coefs[CW], B, CW, True, 50.0, _lib.FFT_F32, coffs, cen, RADIUS, STEP, True, *args, o, mem))
    env = np.zeros(CW * int(offs[-1]))
    ctx.filterbank_envelope_fused(i16, _lib.WAVE_I16, offs, coefs[CW], B, CW, True, 50.0, _lib.FFT_F32, env, None, _lib.MEM_HOST)
    for vname, mof in (("every utterance mixed or sharp by its level", mix_of), ("all sharp", idle["all sharp"]["mix_of"]), ("no levels", None)):
        for norm in (True, False):
            both(f"f2_gather_windows_mixed: {vname}, normalize {int(norm)}", env, n * R * CW, lambda mem, e, o: ctx.gather_windows_mixed(
                e, offs, B, CW, coffs, cen, RADIUS, STEP, norm, mix, mof, o, mem))
    print("window outputs done", flush=True)

    # a trainer in groups of two over five utterances (the middle group: one utterance without windows), each render and one pass of
    # steps behind the last
    lens5 = lens + [2100, 1900]
    w5 = [orc.synth_utterance(4300 + i, m).astype(np.int16) for i, m in enumerate(lens5)]
    cs5 = [np.array([reach, m - 1 - reach], np.int64) if m > 2 * reach else np.zeros(0, np.int64) for m in lens5]
    sg5 = [(np.arange(len(c)) % 2).astype(np.uint8) for c in cs5]
    room5, lev5, mof5 = np.array([1, 2, 0, 2, 0], np.int32), np.array([0, 2, 1, 2, 1], np.int32), np.array([2, 0, 1, 3, 1], np.int32)
    mix5 = mixes(CT)
    tr = Trainer(F2CNNModel.glorot(7, R, CT, zero_bias=False), lr=1e-3, decay=1e-6, drop=(0.25, 0.25, 0.5), seed=5, ctx=ctx)
    tr.set_waves(w5, cs5, sg5, coefs[CT], RADIUS, STEP, lpf=True, group=2)
    renders = [("render", lambda: tr.render(snr, lev5, seed)), ("render_wet", lambda: tr.render_wet(rirs, room5, snr, lev5, seed)),
               ("render(firs=)", lambda: tr.render(snr, lev5, seed, firs=firs)),
               ("render_wet(mixes=)", lambda: tr.render_wet(rirs, room5, snr, lev5, seed, firs=firs, mixes=mix5, mix_of=mof5))]
    for rname, render in renders:
        render()
        res[f"f2_trainer_{rname}: five utterances in groups of two, the rendered windows"] = digest(*tr.windows())
    nw = len(tr.windows()[1])
    loss, hits = tr.steps(np.random.default_rng(5).permutation(nw), 4)
    res["f2_trainer_steps behind render_wet(mixes=): weights, accumulators, gradient, loss, hits"] = digest(
        *tr.weights().values(), *tr.accumulators().values(), *tr.gradient().values(), np.float64(loss), np.int64(hits), np.int64(tr.iterations))
    print("renders done", flush=True)

    # invalid calls: status and message
    p = lambda a: None if a is None else a.ctypes.data
    rir, ro = _lib._pack_rirs(rirs)
    fir, fo = _lib._pack_rirs(firs)
    out = np.zeros(n * R * CW, np.float32)
    dec, far = offs.copy(), cen.copy()
    dec[2], far[0] = dec[1] - 1, 0
    bad_room, bad_level, bad_mof = room_of.copy(), level_of.copy(), mix_of.copy()
    bad_room[2], bad_level[1], bad_mof[2] = KR + 1, K + 1, KM + 1
    nan_rir, nan_fir, nan_mix, nan_snr, fo_long = rir.copy(), fir.copy(), mix.copy(), snr.copy(), fo.copy()
    nan_rir[5], nan_fir[2], nan_mix[1, 4, 5], nan_snr[1], fo_long[2] = np.nan, np.nan, np.nan, np.nan, fo[1] + 2049

    def invalid(name, call, cases):
        rows = []
        for cname, kw in cases:
            rc = call(**kw)
            rows.append(f"{cname}: {rc} {ctx.lib.f2_last_error(ctx.handle).decode()}")
            assert rc != _lib.F2_OK, (name, cname)
        res[f"{name}: {len(cases)} invalid calls, status and message"] = digest(np.frombuffer("\n".join(rows).encode(), np.uint8))

    def smeared(symbol):
        """the call of f2_input_batch_<symbol> with the arguments that symbol has"""
        def call(wave=i16, dt=_lib.WAVE_I16, off=offs, c=CW, cutoff=50.0, centres=cen, rir=rir, ro=ro, kr=KR, room=room_of, s=snr, fir=fir, fo=fo,
                 k=K, level=level_of, mix=mix, km=KM, mof=mix_of, out=out, mem=_lib.MEM_HOST):
            rooms, noise = (p(rir), p(ro), kr, p(room)), (k, p(level), first, seed)      # (the order of include/f2cnn_hip.h, written out)
            stages = {"noisy": (p(s), *noise), "wet": (*rooms, p(s), *noise), "coloured": (*rooms, p(s), p(fir), p(fo), *noise),
                      "smeared": (*rooms, p(s), p(fir), p(fo), *noise, p(mix), km, p(mof))}[symbol]
            return getattr(ctx.lib, "f2_input_batch_" + symbol)(
                ctx.handle, p(wave), dt, p(off), p(coefs[CW]), B, c, 1, cutoff, _lib.FFT_F32, p(coffs), p(centres), RADIUS, STEP, 1,
                *stages, p(out), mem)
        return call
    noise_cases = [("level high", dict(level=bad_level)), ("K<0", dict(k=-1)), ("snr NULL", dict(s=None)), ("snr nan", dict(s=nan_snr)),
                   ("window outside", dict(centres=far)), ("offsets decreasing", dict(off=dec)), ("wave NULL", dict(wave=None)),
                   ("windows NULL", dict(out=None)), ("wave_dtype", dict(dt=7)), ("mem_space", dict(mem=9)), ("C=0", dict(c=0)),
                   ("cutoff", dict(cutoff=9000.0)),
                   # two things wrong at once, in the order of the checks: which one the call names
                   ("mem_space and wave_dtype", dict(mem=9, dt=7)), ("wave_dtype and C=0", dict(dt=7, c=0)), ("C=0 and K<0", dict(c=0, k=-1)),
                   ("level high and offsets decreasing", dict(level=bad_level, off=dec)),
                   ("offsets decreasing and window outside", dict(off=dec, centres=far))]
    room_cases = [("room high", dict(room=bad_room)), ("rir NULL", dict(rir=None)), ("Kr<0", dict(kr=-1)), ("rir tap nan", dict(rir=nan_rir)),
                  ("rir_offsets NULL", dict(ro=None)), ("window outside and room high", dict(centres=far, room=bad_room)),
                  ("level high and room high", dict(level=bad_level, room=bad_room))]
    colour_cases = [("fir_offsets NULL", dict(fo=None)), ("fir tap nan", dict(fir=nan_fir)),
                    ("2049 taps", dict(fir=np.ones(int(fo_long[2])), fo=fo_long)), ("window outside and fir tap nan", dict(centres=far, fir=nan_fir)),
                    ("fir tap nan and room high", dict(fir=nan_fir, room=bad_room)), ("fir tap nan and rir NULL", dict(fir=nan_fir, rir=None))]
    mix_cases = [("mix NULL", dict(mix=None)), ("weight nan", dict(mix=nan_mix)), ("mix level high", dict(mof=bad_mof)), ("Km<0", dict(km=-1)),
                 ("Km=65", dict(mix=np.resize(mix, (65, CW, CW)), km=65)), ("room high and weight nan", dict(room=bad_room, mix=nan_mix)),
                 ("rir tap nan and Km<0", dict(rir=nan_rir, km=-1)), ("weight nan and mix level high", dict(mix=nan_mix, mof=bad_mof))]
    invalid("f2_input_batch_noisy", smeared("noisy"), noise_cases)
    invalid("f2_input_batch_wet", smeared("wet"), noise_cases + room_cases)
    invalid("f2_input_batch_coloured", smeared("coloured"), noise_cases + room_cases + colour_cases)
    invalid("f2_input_batch_smeared", smeared("smeared"), noise_cases + room_cases + colour_cases + mix_cases)

    def gather(env=env, off=offs, c=CW, centres=cen, mix=mix, km=KM, mof=mix_of, out=out, mem=_lib.MEM_HOST, nb=B):
        return ctx.lib.f2_gather_windows_mixed(ctx.handle, p(env), p(off), nb, c, p(coffs), p(centres), RADIUS, STEP, 1, p(mix), km, p(mof),
                                               p(out), mem)
    invalid("f2_gather_windows_mixed", gather, [
        ("mem_space", dict(mem=9)), ("C=0", dict(c=0)), ("B<0", dict(nb=-1)), ("Km<0", dict(km=-1)), ("mix NULL", dict(mix=None)),
        ("weight nan", dict(mix=nan_mix)), ("mix level high", dict(mof=bad_mof)), ("offsets decreasing", dict(off=dec)),
        ("window outside", dict(centres=far)), ("env NULL", dict(env=None)), ("windows NULL", dict(out=None)),
        ("mem_space and C=0", dict(mem=9, c=0)), ("C=0 and Km<0", dict(c=0, km=-1)), ("mix level high and offsets decreasing", dict(mof=bad_mof, off=dec)),
        ("offsets decreasing and window outside", dict(off=dec, centres=far))])

    bad_room5, bad_lev5, bad_mof5, nan_mix5 = room5.copy(), lev5.copy(), mof5.copy(), mix5.copy()
    bad_room5[4], bad_lev5[3], bad_mof5[3], nan_mix5[1, 2, 3] = KR + 1, K + 1, KM + 1, np.nan

    bare = Trainer(F2CNNModel.glorot(7, R, CT, zero_bias=False), ctx=ctx)      # (no set_waves)

    def render(symbol):
        def call(rir=rir, ro=ro, kr=KR, room=room5, s=snr, fir=fir, fo=fo, k=K, level=lev5, mix=mix5, km=KM, mof=mof5, t=tr.handle):
            rooms, noise = (p(rir), p(ro), kr, p(room)), (k, p(level), seed)
            stages = {"": (p(s), *noise), "_wet": (*rooms, p(s), *noise), "_coloured": (*rooms, p(s), p(fir), p(fo), *noise),
                      "_smeared": (*rooms, p(s), p(fir), p(fo), *noise, p(mix), km, p(mof))}[symbol]
            return getattr(ctx.lib, "f2_trainer_render" + symbol)(ctx.handle, t, *stages)
        return call
    r_noise = [("level high", dict(level=bad_lev5)), ("snr nan", dict(s=nan_snr)), ("snr NULL", dict(s=None)), ("K<0", dict(k=-1, level=None)),
               ("trainer NULL", dict(t=None)), ("trainer NULL and K<0", dict(t=None, k=-1)), ("trainer without waves", dict(t=bare.handle)),
               ("trainer without waves and K<0", dict(t=bare.handle, k=-1, level=None))]
    r_room = [("room high", dict(room=bad_room5)), ("rir NULL", dict(rir=None)), ("Kr<0", dict(kr=-1)), ("rir tap nan", dict(rir=nan_rir)),
              ("level high and room high", dict(level=bad_lev5, room=bad_room5))]
    r_colour = [("fir_offsets NULL", dict(fo=None)), ("fir tap nan", dict(fir=nan_fir)), ("level high and fir tap nan", dict(level=bad_lev5, fir=nan_fir)),
                ("fir tap nan and room high", dict(fir=nan_fir, room=bad_room5))]
    r_mix = [("mix level high", dict(mof=bad_mof5)), ("weight nan", dict(mix=nan_mix5)), ("mix NULL", dict(mix=None)), ("Km<0", dict(km=-1)),
             ("room high and weight nan", dict(room=bad_room5, mix=nan_mix5)), ("weight nan and mix level high", dict(mix=nan_mix5, mof=bad_mof5))]
    invalid("f2_trainer_render", render(""), r_noise)
    invalid("f2_trainer_render_wet", render("_wet"), r_noise + r_room)
    invalid("f2_trainer_render_coloured", render("_coloured"), r_noise + r_room + r_colour)
    invalid("f2_trainer_render_smeared", render("_smeared"), r_noise + r_room + r_colour + r_mix)
    res["f2_trainer_render_*: the windows after the invalid calls"] = digest(*tr.windows())
    tr.close()
    bare.close()
    print("window cases done", flush=True)


def keep_arrays(keep, key, arrays, lens=None, C=None, envelopes=()):
    """the outputs of one case under KEEP_DIR: a<i>.npy each; `envelopes` = the indices of the arrays laid out
    [utterance][channel][sample] for utterances of `lens` samples and C channels"""
    if not keep:
        return
    d = os.path.join(keep, hashlib.sha256(key.encode()).hexdigest()[:16])
    os.makedirs(d, exist_ok=True)
    for i, a in enumerate(arrays):
        np.save(os.path.join(d, f"a{i}.npy"), np.ascontiguousarray(a))
    with open(os.path.join(d, "layout.json"), "w") as f:
        json.dump({"case": key, "lens": lens, "C": C, "is_envelope": [i in envelopes for i in range(len(arrays))]}, f)


def worst_row_difference(key, old_keep, new_keep):
    """max over the kept arrays and their rows of max |new - old| / max |old| (None without kept outputs of this case)"""
    d = hashlib.sha256(key.encode()).hexdigest()[:16]
    lay = os.path.join(old_keep, d, "layout.json")
    if not os.path.exists(lay) or not os.path.exists(os.path.join(new_keep, d, "a0.npy")):
        return None
    with open(lay) as f:
        lay = json.load(f)
    worst = 0.0
    for i, is_env in enumerate(lay["is_envelope"]):
        a = np.load(os.path.join(old_keep, d, f"a{i}.npy")).astype(np.float64)
        b = np.load(os.path.join(new_keep, d, f"a{i}.npy")).astype(np.float64)
        if is_env:
            o = 0
            for n in lay["lens"]:
                ra, rb = a.ravel()[o:o + lay["C"] * n].reshape(lay["C"], n), b.ravel()[o:o + lay["C"] * n].reshape(lay["C"], n)
                o += lay["C"] * n
                worst = max(worst, float((np.abs(rb - ra).max(axis=1) / np.maximum(np.abs(ra).max(axis=1), 1e-300)).max()))
        elif a.size:
            worst = max(worst, float(np.abs(b - a).max() / max(np.abs(a).max(), 1e-300)))
    return worst


def run(lib, out, keep=None, only=None):
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(lib)
    import f2cnn_oracle as orc
    from f2cnn_amd import _lib
    from f2cnn_amd.model import F2CNNModel
    ctx = _lib.Context(0)
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))
    h = F2CNNModel.glorot(11).handle(ctx)
    res = {}
    for name, lens in BATCHES if not only else []:
        waves = [orc.synth_utterance(500 + i, n) for i, n in enumerate(lens)]
        flat = np.concatenate(waves)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        B, total = len(lens), int(offs[-1])
        nbs = [max(n - R * STEP, 0) for n in lens]
        # two centres per utterance that has room for a window: the first and the last legal one
        cs = [np.array([RADIUS * STEP, n - 1 - RADIUS * STEP], np.int64) if n > 2 * RADIUS * STEP else np.zeros(0, np.int64) for n in lens]
        coffs = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
        for lpf in (False, True):
            cut = 50.0 if lpf else 0.0
            tag = f"{name}, {'LPF 50 Hz' if lpf else 'no LPF'}"
            env = np.zeros((C * total,))
            ctx.filterbank_envelope_fused(flat, _lib.WAVE_I16, offs, coefs, B, C, lpf, cut, _lib.FFT_F32, env, None, _lib.MEM_HOST)
            res[f"f2_filterbank_envelope_fused: {tag}"] = digest(env)
            if lpf:
                keep_arrays(keep, f"f2_filterbank_envelope_fused: {tag}", [env], lens, C, envelopes=(0,))
            sc, lb = np.zeros((sum(nbs), 2), np.float32), np.zeros(sum(nbs), np.uint8)
            ctx.eval_batch(h, flat, _lib.WAVE_I16, offs, coefs, B, C, lpf, cut, _lib.FFT_F32, RADIUS, STEP, sc, lb, _lib.MEM_HOST)
            res[f"f2_eval_batch: {tag}"] = digest(sc, lb)
            if lpf:
                keep_arrays(keep, f"f2_eval_batch: {tag}", [sc, lb])
            if B == 1:
                sc, lb, env = np.zeros((nbs[0], 2), np.float32), np.zeros(nbs[0], np.uint8), np.zeros((C, total))
                nb = ctx.eval_utterance(h, flat, _lib.WAVE_I16, total, coefs, C, lpf, cut, _lib.FFT_F32, RADIUS, STEP, env, sc, lb,
                                        _lib.MEM_HOST)
                res[f"f2_eval_utterance: {tag}"] = digest(sc, lb, env, np.int64(nb))
                if lpf:
                    keep_arrays(keep, f"f2_eval_utterance: {tag}", [env, sc, lb], lens, C, envelopes=(0,))
            win = np.zeros((int(coffs[-1]), R, C), np.float32)
            ctx.input_batch(flat, _lib.WAVE_I16, offs, coefs, B, C, lpf, cut, _lib.FFT_F32, coffs,
                            np.concatenate(cs) if len(cs) else np.zeros(0, np.int64), RADIUS, STEP, True, win, _lib.MEM_HOST)
            res[f"f2_input_batch: {tag}"] = digest(win)
            if lpf:
                keep_arrays(keep, f"f2_input_batch: {tag}", [win])
            print(tag, "done", flush=True)
    for group in (cnn_cases, entry_cases, sweep_cases, grad_cases, figure_cases, stage_cases, window_cases):
        if not only or group.__name__ in only.split(","):
            group(ctx, res)
    ctx.close()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def compare(a, b, old_keep=None, new_keep=None):
    with open(a) as fa, open(b) as fb:
        old, new = json.load(fa), json.load(fb)
    assert list(old) == list(new)
    bad, worst = 0, 0.0
    for k in old:
        same = old[k] == new[k]
        bad += not same
        note = ""
        if not same and old_keep and new_keep:
            w = worst_row_difference(k, old_keep, new_keep)
            if w is not None:
                worst = max(worst, w)
                note = f", largest difference relative to the row maximum {w:.3g}"
        print(f"{k}: {'identical' if same else 'DIFFERS'} ({old[k]}{'' if same else ' / ' + new[k]}){note}")
    print(f"{len(old) - bad} of {len(old)} cases identical")
    if bad and old_keep and new_keep:
        print(f"largest difference relative to the row maximum over the cases that differ: {worst:.3g}")
    return 1 if bad else 0


if __name__ == "__main__":
    only = [a[len("--only="):] for a in sys.argv if a.startswith("--only=")]
    args = [a for a in sys.argv if not a.startswith("--only=")]
    sys.exit(run(*args[2:5], only=only[0] if only else None) if args[1] == "run" else compare(*args[2:6]))
