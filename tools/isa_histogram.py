"""Static instruction histogram of one kernel in a `hipcc -S` listing (CPU only, no GPU needed):

    hipcc -O3 -std=c++17 -fno-slp-vectorize --offload-arch=gfx950 --cuda-device-only -S f2cnn_amd/csrc/f2_spectral.hip -o ks.s
    python tools/isa_histogram.py ks.s 'k_spectral_envelope.*Li13.*Lb1'

The pattern is a regular expression searched in the (mangled) symbol names; every matching kernel is reported.
Instructions are classified by their prefix alone - `v_` (vector ALU), `ds_` (LDS), `s_barrier` - and the vector ones are
split into float32 arithmetic (mnemonic `v_<op>_f32`, encoding suffixes `_e32` / `_e64` / `_dpp` / `_sdwa` stripped; conversions
`v_cvt_*`, comparisons `v_cmp*`, selects and moves count as "other") and everything else by opcode. Static counts: a loop body counts once.
"""
import collections
import re
import sys

ENCODING = re.compile(r"_(e32|e64|sdwa)$")
F32_ARITH = re.compile(r"^v_(?!cvt_|cmp|cndmask|mov_)[a-z0-9]+_f32$")


def kernels(text):
    """{symbol: [mnemonic, ...]} for every function body between `sym:` and `.Lfunc_end`"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_][\w.$]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        cur.append(s.split()[0])
    return out


def classify(mnemonics):
    """(float32-arithmetic counter, other-VALU counter, LDS counter, barriers) of a list of mnemonics"""
    f32, other, lds, barriers = collections.Counter(), collections.Counter(), collections.Counter(), 0
    for op in mnemonics:
        if op.startswith("s_barrier"):
            barriers += 1
        elif op.startswith("ds_"):
            lds[op] += 1
        elif op.startswith("v_"):
            base = ENCODING.sub("", op)
            dpp = base.endswith("_dpp")
            stem = base[:-4] if dpp else base
            if F32_ARITH.match(stem):
                f32[base] += 1
            else:
                other[base] += 1
    return f32, other, lds, barriers


def report(name, mnemonics, out=sys.stdout):
    f32, other, lds, barriers = classify(mnemonics)
    nf, no, nl = sum(f32.values()), sum(other.values()), sum(lds.values())
    print(f"== {name}", file=out)
    print(f"VALU {nf + no}  (float32 arithmetic {nf}, other {no})   LDS {nl}   barriers {barriers}", file=out)
    for title, cnt in (("float32 arithmetic", f32), ("other VALU", other), ("LDS", lds)):
        print(f"  {title}:", file=out)
        for op, k in sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0])):
            print(f"    {k:6d}  {op}", file=out)


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    with open(argv[1]) as f:
        ks = kernels(f.read())
    pat = re.compile(argv[2])
    hits = [k for k in ks if pat.search(k) and ks[k]]
    if not hits:
        print(f"no kernel matches {argv[2]!r}; symbols: " + ", ".join(k for k in ks if ks[k]), file=sys.stderr)
        return 1
    for k in hits:
        report(k, ks[k])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
