"""Device code of the working tree against a commit's, translation unit by translation unit. No GPU is needed.
    python tools/device_code_identity.py [REV]        (REV: the commit to compare with, default HEAD)
    python tools/device_code_identity.py [REV] --kernels [OLD.hip=NEW.hip ...]
Every csrc/*.hip of REV (from `git archive`, in a temporary directory) and of the tree is compiled with the flags of its own
f2cnn_amd/build.py (per-file flags included) plus --cuda-device-only -S. The two listings are compared whole, line by line,
after masking the __hip_cuid_<hash> symbol (a hash of path and options) and the listing's own path; one line per file is
printed. A host-only change to a file that holds kernels must leave its line at "identical". Exit status 1 if a file differs.

--kernels is for a change that renames kernels (a namespace, a template parameter) or moves them between files without
touching their code. The listings are cut at the function symbols; a kernel's text runs from its label to the end of its
"Kernel info" block (instruction stream, .amdhsa_ descriptor, register / LDS / scratch figures) and is followed by its entry
in the metadata note. Inside it the kernel's own mangled name, every other mangled symbol (numbered in order of appearance)
and the function index in local labels (.LBB<i>_, .Lfunc_end<i>) are masked. Every kernel of an old file must then have a
counterpart with the same text in the new file of the same name, or in the one an OLD.hip=NEW.hip argument names (several
old files may share a new one); matching is by text, names are only reported. A new kernel that no old one claims counts
as a difference too. A file that is neither side of an explicit mapping must in addition be identical as a whole listing
under the same masking (symbols numbered over the file)."""
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


def mask_symbols(lines, own=None):
    """`own` -> KERNEL, other mangled symbols -> _Zsym<order of appearance>, function indices out of local labels"""
    seen = {}

    def sym(m):
        return "KERNEL" if m.group(0) == own else seen.setdefault(m.group(0), f"_Zsym{len(seen)}")

    out = []
    for l in lines:
        l = re.sub(r"\b_Z\w+", sym, l)
        l = re.sub(r"\bL?BB\d+_", "BB_", l)
        l = re.sub(r"^(\.BB_\d+:)\s+;", r"\1 ;", l)   # (the comment column moves with the width of the index)
        out.append(re.sub(r"\bLfunc_(begin|end)\d+", r"Lfunc_\1", l))
    return out


def kernels(lines):
    """{mangled name: (masked text, figures)} of every function of a listing, in listing order"""
    meta, name_at = {}, None
    if "\t.amdgpu_metadata" in lines:
        a = lines.index("\t.amdgpu_metadata")
        entry = []
        for l in lines[a:] + ["  - "]:
            if l.startswith("  - ") or not l.startswith("    "):
                name = next((e.split()[1] for e in entry if e.startswith("    .name:")), None)
                if name:
                    meta[name] = entry
                entry = []
            entry.append(l)
    out = {}
    starts = [i for i, l in enumerate(lines) if "; -- Begin function " in l]
    for i in starts:
        name = lines[i].split("; -- Begin function ")[1].strip()
        end = next(j for j in range(i, len(lines)) if "; -- End function" in lines[j]) + 1
        while end < len(lines) and (lines[end].startswith(("\t.set ", ";")) or ".AMDGPU.csdata" in lines[end]):
            end += 1
        text = mask_symbols(lines[i:end] + meta.get(name, []), name)
        fig = {k: next((l.split(":")[1].split()[0] for l in lines[i:end] if l.startswith(f"; {k}:")), "-")
               for k in ("NumVgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize")}
        out[name] = (text, f"VGPRs {fig['NumVgprs']}, SGPRs {fig['TotalNumSgprs']}, LDS {fig['LDSByteSize']} B, scratch {fig['ScratchSize']} B")
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True)
    short = [re.sub(r"\(anonymous namespace\)::|\(.*", "", s) for s in res.stdout.splitlines()] if res.returncode == 0 else names
    return dict(zip(names, short))


def compare_kernels(old_l, new_l, mapping):
    """prints one line per kernel; returns the number of differences"""
    bad = 0
    new_k = {n: kernels(l.result()) for n, l in new_l.items()}
    claimed = {n: set() for n in new_k}
    mapped = set(mapping) | set(mapping.values())
    for name in sorted(old_l):
        target = mapping.get(name, name)
        old_k = kernels(old_l[name].result())
        if target not in new_k:
            print(f"{name}: only in the commit ({len(old_k)} kernels)")
            bad += 1
            continue
        pretty = demangle(list(old_k) + list(new_k[target]))
        print(f"{name} -> {target}: {len(old_k)} kernels")
        for k, (text, fig) in old_k.items():
            free = [n for n in new_k[target] if n not in claimed[target]]
            hit = next((n for n in free if new_k[target][n][0] == text), None)
            if hit:
                claimed[target].add(hit)
                print(f"  {pretty[k]} = {pretty[hit]}: identical ({len(text)} lines; {fig})")
                continue
            bad += 1
            near = max(free, key=lambda n: difflib.SequenceMatcher(None, pretty[k], pretty[n]).ratio(), default=None)
            if near is None:
                print(f"  {pretty[k]}: NO COUNTERPART ({fig})")
                continue
            other, ofig = new_k[target][near]
            delta = [l for l in difflib.unified_diff(text, other, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            print(f"  {pretty[k]}: DIFFERS from {pretty[near]} ({len(delta)} changed lines of {len(text)} / {len(other)}; {fig} / {ofig}), "
                  f"first: {delta[0][:100] if delta else ''}")
        if name not in mapped:
            same = name in new_l and mask_symbols(old_l[name].result()) == mask_symbols(new_l[name].result())
            print(f"  whole listing: {'identical' if same else 'DIFFERS'}")
            bad += not same
    for n in sorted(new_k):
        left = [k for k in new_k[n] if k not in claimed[n]]
        if left:
            pretty = demangle(left)
            print(f"{n}: {len(left)} kernels of the tree without a counterpart in the commit: {', '.join(pretty.values())}")
            bad += len(left)
    return bad


def main():
    args = sys.argv[1:]
    per_kernel = "--kernels" in args
    mapping = dict(a.split("=") for a in args if "=" in a)
    revs = [a for a in args if a != "--kernels" and "=" not in a]
    rev = revs[0] if revs else "HEAD"
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
        if per_kernel:
            print("per kernel, mangled names masked" + "".join(f"; {o} -> {n}" for o, n in mapping.items()))
            bad = compare_kernels(old_l, new_l, mapping)
            print("every kernel of the commit has an identical counterpart in the tree" if not bad else f"{bad} differences")
            return 1 if bad else 0
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
