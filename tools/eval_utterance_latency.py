"""Device time of f2_eval_utterance on one long utterance (default 40 000 and 64 000 samples, 128 channels, device memory):
HIP-event time over 20 calls after 5 warm-up calls, per call. F2CNN_PROBE_LIB picks another build of the library. Diagnostic."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.gammatone import filters
from f2cnn_amd.model import F2CNNModel
import bench

C, RADIUS, STEP = 128, 5, 160
ctx = _lib.Context(0)
coefs = filters.make_erb_filters(16000, filters.centre_freqs(16000, C, 100))
h = F2CNNModel.glorot(11).handle(ctx)
for N in [int(a) for a in sys.argv[1:]] or [40000, 64000]:
    wave = bench.synth_batch(1234, 0, 1, N)
    nb = N - (2 * RADIUS + 1) * STEP
    d_wave = ctx.malloc(wave.nbytes); ctx.h2d(d_wave, wave)
    d_scores, d_labels = ctx.malloc(8 * nb), ctx.malloc(nb)
    run = lambda: ctx.eval_utterance(h, d_wave, _lib.WAVE_I16, N, coefs, C, True, 50.0, _lib.FFT_F32, RADIUS, STEP, None, d_scores,
                                     d_labels, _lib.MEM_DEVICE)
    for _ in range(5):
        run()
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(20):
        run()
    ctx.record(e1)
    ms = ctx.elapsed_ms(e0, e1) / 20
    print(f"eval_utterance {N} samples ({nb} windows): {ms:.4f} ms per call", flush=True)
    for ev in (e0, e1):
        ctx.destroy_event(ev)
    for p in (d_wave, d_scores, d_labels):
        ctx.free(p)
ctx.close()
