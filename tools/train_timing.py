"""One training epoch on windows resident on the device: `cnn train --engine hip` (f2_trainer_steps) against `--engine torch`
(PyTorch-ROCm autograd, the code of Training._torch_engine), same process, alternating, a warm epoch of each first, host clock
around work that ends in a device synchronise, median of --repeats.

    python3 tools/train_timing.py [--windows 65536] [--batches 32,256] [--repeats 3] [--out profiles/r26_train_timing.json]
    rocprofv3 --kernel-trace --stats -- python3 tools/train_timing.py --only-hip --windows 8192 --batches 256 --repeats 1
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from f2cnn_amd.model import F2CNNModel                      # noqa: E402
from f2cnn_amd.scripts.CNN import Training                   # noqa: E402
from f2cnn_amd.trainer import Trainer                        # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    rows, channels, seed = 11, 128, 3
    rng = np.random.default_rng(seed)
    x = rng.random((a.windows, rows, channels), dtype=np.float32)     # (normalised windows lie in [0, 1])
    y = rng.integers(0, 2, a.windows).astype(np.uint8)
    result = {"workload": "one epoch of {} normalised {}x{} windows resident on the device".format(a.windows, rows, channels),
              "clock": "time.perf_counter around one epoch ending in a device synchronise; median of {} after a warm epoch".format(a.repeats),
              "batches": {}}
    for batch in [int(b) for b in a.batches.split(",")]:
        trainer = Trainer(F2CNNModel.glorot(seed, rows, channels), lr=1e-4, decay=1e-6, drop=Training.DROPOUT, seed=seed)
        trainer.set_data(x, y)

        def hip_epoch():
            t0 = time.perf_counter()
            trainer.steps(rng.permutation(a.windows), batch)          # (returns after its one wait for the stream)
            return time.perf_counter() - t0

        engines = {"hip": hip_epoch}
        if not a.only_hip:
            import torch
            run_epoch, _, _ = Training._torch_engine(x, y, x[:0], y[:0], batch, None, seed, 1e-4, 1e-6)

            def torch_epoch():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_epoch()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            engines["torch"] = torch_epoch
        times = {k: [] for k in engines}
        for k, fn in engines.items():
            fn()                                                      # warm
        for _ in range(a.repeats):
            for k, fn in engines.items():                             # alternating
                times[k].append(fn())
        entry = {k: {"seconds": v, "median_s": statistics.median(v), "windows_per_s": a.windows / statistics.median(v),
                     "ms_per_step": 1e3 * statistics.median(v) / -(-a.windows // batch)} for k, v in times.items()}
        if "torch" in entry:
            entry["hip_over_torch_rate"] = entry["torch"]["median_s"] / entry["hip"]["median_s"]
        result["batches"][str(batch)] = entry
        trainer.close()
        print("batch {}: {}".format(batch, json.dumps(entry)), flush=True)
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
