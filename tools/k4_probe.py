"""K4 probe: the CNN forward pass on 4096 device-resident windows, 10 launches. Run under
`rocprofv3 --kernel-trace --stats` for per-layer times; F2CNN_PROBE_LIB picks a tools/build_variant.sh library.
    python tools/k4_probe.py [n] [--f32] [--shape ROWSxCHANNELS]
--f32 sets the option cnn_f16x3 = 0 (the float32 matrix-core kernels; layer by layer where the window does not have four
pooled rows), --shape another window than 11x128."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("F2CNN_PROBE_LIB"):
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(os.environ["F2CNN_PROBE_LIB"])
from f2cnn_amd import _lib
from f2cnn_amd.model import F2CNNModel

args = sys.argv[1:]
f32 = "--f32" in args
rows, channels = (int(v) for v in args[args.index("--shape") + 1].split("x")) if "--shape" in args else (11, 128)
plain = [a for k, a in enumerate(args) if not a.startswith("--") and (k == 0 or args[k - 1] != "--shape")]
n = int(plain[0]) if plain else 4096
ctx = _lib.Context(0)
if f32:
    ctx.set_option("cnn_f16x3", 0)
m = F2CNNModel.glorot(7, rows, channels)
h = m.handle(ctx)
x = np.random.default_rng(0).uniform(0, 1, (n, rows, channels)).astype(np.float32)
d_x = ctx.malloc(x.nbytes); ctx.h2d(d_x, x)
d_s = ctx.malloc(8 * n); d_l = ctx.malloc(n)
ctx.cnn_forward(h, d_x, n, d_s, d_l, _lib.MEM_DEVICE); ctx.synchronize()
ctx.prof_enable(True)
for _ in range(10):
    ctx.cnn_forward(h, d_x, n, d_s, d_l, _lib.MEM_DEVICE)
p = ctx.prof_get()
H2, W2 = rows - 2, channels - 2
Hp1, Wp1 = H2 // 2, W2 // 2
flop = 2 * (rows * channels * 9 * 32 + H2 * W2 * 9 * 32 * 32 + Hp1 * Wp1 * 9 * 32 * 64 + (Hp1 - 2) * (Wp1 - 2) * 9 * 64 * 64
            + (Hp1 - 2) // 2 * ((Wp1 - 2) // 2) * 64 * 516 + 516 * 2)      # 41.98e6 for 11 x 128
for k, (c, t) in p.items():
    print(k, f"{t / 10:.3f} ms per forward of {n} windows = {n * flop / (t / 10 * 1e-3) / 1e12:.1f} TFLOP/s", flush=True)
