"""Register table of the decode kernels from the compiler's own remarks.

Usage: hipcc <the Makefile's FLAGS> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
           decode.hip -o decode.s 2> decode.remarks
       python tools/decode_regs.py decode.remarks [decode.s] [--compare OLD.remarks OLD.s]
Prints, per kernel, VGPRs, SGPRs, scratch bytes, occupancy and LDS,
and with the assembly the number of instructions between the kernel's label and its
s_endpgm.  --compare matches the kernels of an older build by name with the cache element
type dropped (decode_kernel<E, N, PG, E> is the old decode_kernel<E, N, PG>) and prints the
rows that differ: the existing instantiations must not gain an instruction."""
import re
import sys


TYPES = {"DF16b": "bf16", "DF16_": "f16", "f": "f32", "NS0_4f8e4E": "f8e4"}


def readable(mangled):
    """decode_split_kernel<bf16,2,64,128,256,1,f8e4> from the Itanium name (c++filt does not know __bf16)."""
    m = re.match(r"_ZN3dta12_GLOBAL__N_1\d+([a-z0-9_]+?)I(.*)EEvNS_\d+\w+Params?E$", mangled)
    if not m:
        return mangled
    args = re.findall(r"DF16b|DF16_|NS0_4f8e4E|f|L[ib]\d+E", m.group(2))
    return m.group(1) + "<" + ",".join(TYPES.get(a, a[2:-1]) for a in args) + ">"


def remarks(path):
    rows, cur = {}, None
    for ln in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}(VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return rows


def instructions(path):
    counts, cur = {}, None
    for ln in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = m.group(1)
            counts[cur] = 0
            continue
        s = ln.strip()
        if cur and s and not s.startswith((".", ";", "//")) and not s.endswith(":"):
            counts[cur] += 1
            if s.startswith("s_endpgm"):
                cur = None
    return counts


def table(rem, asm):
    rows = remarks(rem)
    ins = instructions(asm) if asm else {}
    names = list(rows)
    out = {}
    for mangled in names:
        nice = readable(mangled)
        r = rows[mangled]
        out[nice] = (r.get("VGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize"), r.get("Occupancy"), r.get("LDS"),
                     ins.get(mangled))
    return out


def strip_cache_type(name):
    """decode_split_kernel<E,N,HS,DV,chunk,PG,E> -> <E,N,HS,DV,chunk,PG> (cache type = E only)."""
    m = re.match(r"(decode_(?:split_)?kernel)<(.*)>$", name)
    if not m:
        return name
    args = m.group(2).split(",")
    if len(args) in (4, 7) and args[-1] == args[0]:
        args = args[:-1]
    return f"{m.group(1)}<{','.join(args)}>"


def main():
    argv = sys.argv[1:]
    cmp_ = None
    if "--compare" in argv:
        i = argv.index("--compare")
        cmp_ = argv[i + 1:i + 3]
        argv = argv[:i]
    new = table(argv[0], argv[1] if len(argv) > 1 else None)
    print("kernel | VGPRs | SGPRs | scratch | occupancy | LDS | instructions")
    for k in sorted(new):
        print(k, "|", " | ".join(str(x) for x in new[k]))
    if cmp_:
        old = table(cmp_[0], cmp_[1] if len(cmp_) > 1 else None)
        seen = {strip_cache_type(k): v for k, v in new.items() if "f8e4" not in k}
        bad = [(k, v, seen.get(k)) for k, v in old.items() if seen.get(k) != v]
        print(f"compared {len(old)} existing kernels: {len(bad)} differ")
        for k, a, b in bad:
            print("  ", k, "old", a, "new", b)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
