#!/usr/bin/env python3
"""
Generate tests/golden/f2cnn_golden_gtg.npz by IMPORTING the reference's scripts.plotting.PlottingProcessing (read-only, from the
tree $F2CNN_REFERENCE or the first argument points to). Only data is written: the heights and ERB ratios of three filterbanks
and two small reshaped matrices; no reference source is copied.

    F2CNN_REFERENCE=<reference tree> python tests/golden/make_golden_gtg.py

The module imports matplotlib (MPLBACKEND=Agg: nothing is drawn) and, through GammatoneFiltering, `sphfile`, which is not
installed: the same temp-dir stand-in as make_golden.py's G5 (an SPHFile that refuses to be used) is put on the path for the
import and never written into the repository.
"""
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
REF = os.environ.get("F2CNN_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF or not os.path.isdir(os.path.join(REF, "scripts", "plotting")):
    sys.exit("give the reference tree: F2CNN_REFERENCE=<path> python tests/golden/make_golden_gtg.py  (or the path as argument)")
HERE = os.path.dirname(os.path.abspath(__file__))
BANKS = ((16000, 128, 100), (16000, 64, 100), (16000, 8, 50))


def main():
    os.environ["MPLBACKEND"] = "Agg"
    sys.path.insert(0, REF)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "sphfile.py"), "w") as f:
            f.write("class SPHFile:\n    def __init__(self, *a, **k):\n        raise RuntimeError('sphfile is not installed')\n")
        sys.path.insert(0, tmp)
        try:
            from gammatone import filters as ref_filters
            from scripts.plotting import PlottingProcessing as ref_plot
        finally:
            sys.path.remove(tmp)
    out = {"banks": np.array(BANKS, np.int64)}
    for fs, C, low in BANKS:
        cf = ref_filters.centre_freqs(fs, C, low)
        height, ratios = ref_plot.GetNewHeightERB(np.zeros((C, 1)), cf)
        out[f"cf_{fs}_{C}_{low}"] = cf
        out[f"height_{fs}_{C}_{low}"] = np.array(height, np.int64)
        out[f"ratios_{fs}_{C}_{low}"] = np.array(ratios, np.int64)
        assert min(ratios) > 0, (fs, C, low)
    cf8 = out["cf_16000_8_50"]
    matrix = np.random.default_rng(941).lognormal(0.0, 3.0, (8, 37))
    out["reshape_matrix"] = matrix
    out["reshape_whole"] = ref_plot.ReshapeEnvelopesForSpectrogram(matrix, cf8)
    out["reshape_5_30"] = ref_plot.ReshapeEnvelopesForSpectrogram(matrix, cf8, start=5, end=30)
    path = os.path.join(HERE, "f2cnn_golden_gtg.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: int(v) for k, v in out.items() if k.startswith("height")})


if __name__ == "__main__":
    main()
