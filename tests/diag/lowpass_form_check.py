"""Diagnostic (CPU only): the two float32 formulations of the envelope low-pass, sample by sample, against a float64 lfilter.
    python tests/diag/lowpass_form_check.py [n]
  direct:  y[i] = q y[i-1] + b0 (e[i] + e[i-1])                     (what the kernels scanned before)
  state:   s[i] = q s[i-1] + e[i],  y[i] = b0 (s[i] + s[i-1])       (what they scan now: no neighbour's sample enters)
Every operation is rounded to float32 the way the kernels round it (fused multiply-adds where they use them); the kernels' scan
order differs from this sequential one and both forms here share q and b0 rounded to float32 (which dominates at 5 Hz), so the
figures say how the FORMS compare, not what a kernel's error is. Cutoffs 5, 50 and
100 Hz on a noise envelope, a bursty one and a step; error = max |y - lfilter| / max |lfilter| over the row."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "oracle"))
import f2cnn_oracle as orc

f32 = np.float32


def fma32(a, b, c):
    """float32 fused multiply-add: the exact product and sum in float64 (24 + 24 bits fit), one rounding"""
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def direct(e, q, b0):
    y = np.zeros(len(e), f32)
    yp, ep = f32(0), f32(0)
    for i, x in enumerate(e):
        yp = fma32(q, yp, f32(b0 * f32(x + ep)))
        ep = x
        y[i] = yp
    return y


def state(e, q, b0):
    y = np.zeros(len(e), f32)
    sp = f32(0)
    for i, x in enumerate(e):
        s = fma32(q, sp, x)
        y[i] = f32(b0 * f32(s + sp))
        sp = s
    return y


def envelopes(n):
    rng = np.random.default_rng(7)
    noise = np.abs(rng.standard_normal(n)) * 1000.0
    burst = noise * 1e-3
    burst[n // 3:n // 3 + 400] = noise[:400] * 10.0
    step = np.where(np.arange(n) < n // 2, 50.0, 5000.0)
    return {"noise": noise, "burst": burst, "step": step}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16000
    print(f"n = {n}; error of the float32 forms against float64 lfilter, relative to the row maximum")
    print(f"{'cutoff':>7} {'envelope':>9} {'direct':>10} {'state':>10} {'state/direct':>13}")
    for cutoff in (5.0, 50.0, 100.0):
        b, a = orc.butter1(cutoff)
        q, b0 = f32(-a[1]), f32(b[0])
        for name, e in envelopes(n).items():
            e32 = e.astype(f32)
            ref = orc.low_pass_filter(e32.astype(np.float64), cutoff)
            ed = np.abs(direct(e32, q, b0) - ref).max() / np.abs(ref).max()
            es = np.abs(state(e32, q, b0) - ref).max() / np.abs(ref).max()
            print(f"{cutoff:7g} {name:>9} {ed:10.3g} {es:10.3g} {es / ed:13.2f}")


if __name__ == "__main__":
    main()
