"""Device code of the working tree against a commit's, translation unit by translation unit. No GPU is needed.
    python tools/device_code_identity.py [REV]        (REV: the commit to compare with, default HEAD)
Every csrc/*.hip of REV (from `git archive`, in a temporary directory) and of the tree is compiled with the flags of its own
f2cnn_amd/build.py (per-file flags included) plus --cuda-device-only -S. The two listings are compared whole, line by line,
after masking the __hip_cuid_<hash> symbol (a hash of path and options) and the listing's own path; one line per file is
printed. A host-only change to a file that holds kernels must leave its line at "identical". Exit status 1 if a file differs."""
import concurrent.futures, difflib, importlib.util, io, os, re, subprocess, sys, tarfile, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_build(root):
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(root))), os.path.join(root, "f2cnn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(build, src, tmp):
    """masked device assembly of one source file, as a list of lines"""
    out = os.path.join(tmp, os.path.basename(src) + ".s")
    cmd = [build.hipcc_path(), "-O3", "-std=c++17", "-fPIC", f"--offload-arch={build.ARCH}", "-Wno-unused-function",
           *build.PER_FILE_FLAGS.get(os.path.basename(src), ()), "--cuda-device-only", "-S", src, "-o", out]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{res.stdout}")
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(out).read())
    return [l for l in text.splitlines() if not l.lstrip().startswith((".file", ".ident"))]


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    with tempfile.TemporaryDirectory() as tmp:
        old_root = os.path.join(tmp, "old")
        os.makedirs(old_root)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "f2cnn_amd", "include"], stdout=subprocess.PIPE, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old_root)
        old_b, new_b = load_build(old_root), load_build(ROOT)
        old_src = {os.path.basename(p): p for p in old_b.sources()}
        new_src = {os.path.basename(p): p for p in new_b.sources()}
        os.makedirs(os.path.join(tmp, "o"))
        os.makedirs(os.path.join(tmp, "n"))
        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            old_l = {n: pool.submit(listing, old_b, p, os.path.join(tmp, "o")) for n, p in old_src.items()}
            new_l = {n: pool.submit(listing, new_b, p, os.path.join(tmp, "n")) for n, p in new_src.items()}
        rev_name = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], stdout=subprocess.PIPE, text=True).stdout.strip()
        print(f"device code (hipcc --cuda-device-only -S, {new_b.ARCH}) of the tree against {rev_name}, __hip_cuid_* masked")
        bad = 0
        for name in sorted(set(old_src) | set(new_src)):
            if name not in old_src or name not in new_src:
                print(f"{name}: only in the {'tree' if name in new_src else 'commit'}")
                bad += 1
                continue
            a, b = old_l[name].result(), new_l[name].result()
            if a == b:
                print(f"{name}: identical ({len(a)} lines)")
            else:
                delta = [l for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
                print(f"{name}: DIFFERS ({len(delta)} changed lines of {len(a)} / {len(b)}), first: {delta[0][:120] if delta else ''}")
                bad += 1
        print(f"{len(new_src) - bad} of {len(new_src)} translation units identical")
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
