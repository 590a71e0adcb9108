"""Diagnostic: bench.py --full against another build of the library (tools/build_variant.sh):
python tools/bench_with_lib.py LIB [bench args]. (--full: the A/B scripts read the per-kernel times; F2CNN_BENCH_PLAIN=1: the
plain line instead.)"""
import os
import sys

if __name__ == "__main__":      # (bench.py starts worker processes that import the main module again)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(sys.argv[1])
    sys.argv = ["bench.py"] + ([] if os.environ.get("F2CNN_BENCH_PLAIN") == "1" else ["--full"]) + sys.argv[2:]
    import bench
    bench.main()
