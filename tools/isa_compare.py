#!/usr/bin/env python3
"""Compare two builds' gfx950 device code kernel by kernel (profiles/*/isa.txt).

  tools/isa_compare.py PARENT.s NEW.s [PARENT2.s NEW2.s ...]

Each .s is `hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S` of one unit.
A kernel is identical when its instruction stream, with labels, directives and comments stripped
(and the function's number taken out of its branch targets), equals the parent's.  p/n = parent /
new; occ = waves per SIMD the compiler states (.amdhsa_next_free_vgpr: 512 registers a lane,
granule 8, at most 8 waves).  A template that gained trailing parameters is paired with the
parent's kernel where the added arguments are all 0; kernels only one build has are listed with
the other side empty.  Exit status 1 if a compared kernel differs.
"""
import os
import re
import subprocess
import sys


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def kernels(path):
    """{symbol: (instructions, scratch, lds, next_free_vgpr)} of every .amdhsa_kernel of the file."""
    body, cur, meta, desc = {}, None, {}, None
    for ln in open(path):
        s = ln.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            desc = m.group(1)
            meta[desc] = {}
            continue
        if desc:
            if s == ".end_amdhsa_kernel":
                desc = None
            else:
                p = s.split()
                if len(p) == 2 and p[0] in (".amdhsa_next_free_vgpr", ".amdhsa_group_segment_fixed_size",
                                            ".amdhsa_private_segment_fixed_size"):
                    meta[desc][p[0]] = int(p[1], 0)
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):", s)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
            body[cur] = []
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None or not s or s.startswith(".") or s.endswith(":"):
            continue
        # a branch target carries its function's number in the unit, which shifts when a kernel is added
        body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)))
    out = {}
    for k, md in meta.items():
        out[k] = (body.get(k, []), md.get(".amdhsa_private_segment_fixed_size", 0),
                  md.get(".amdhsa_group_segment_fixed_size", 0), md.get(".amdhsa_next_free_vgpr", 0))
    return out


def occ(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8)) if vgpr else 8


def main(argv):
    rows, same, diff, only = [], 0, 0, 0
    for pa, nw in zip(argv[0::2], argv[1::2]):
        a, b = kernels(pa), kernels(nw)
        names = demangle(sorted(set(a) | set(b)))
        # a template that gained trailing parameters: the new build's instantiation whose added
        # arguments are all 0 is the parent's kernel under a longer name
        short = {}
        for sym in set(b) - set(a):
            m = re.match(r"^(.*<.*?)((?:, 0)+)>(\(.*)$", names[sym])
            while m:
                short.setdefault(m.group(1) + m.group(2)[:-3] + ">" + m.group(3), sym)
                m = re.match(r"^(.*<.*?)((?:, 0)+)>(\(.*)$", m.group(1) + m.group(2)[:-3] + ">" + m.group(3))
        for sym in set(a) - set(b):
            new = short.get(names[sym])
            if new in b:
                b[sym] = b.pop(new)
                names.pop(new)
        for sym in sorted(names, key=lambda x: names[x]):
            p, n = a.get(sym), b.get(sym)
            name = re.sub(r"^void rsmi::|\(.*$", "", names[sym])
            if p and n:
                ident = p[0] == n[0]
                same += ident
                diff += not ident
                rows.append("%s | %s | %s | %d/%d | %d/%d | %d/%d | %d/%d | %d/%d" % (
                    name, os.path.basename(nw), "yes" if ident else "NO", p[1], n[1], p[2], n[2], p[3], n[3],
                    occ(p[3]), occ(n[3]), len(p[0]), len(n[0])))
            else:
                only += 1
                x = p or n
                side = "%s/-" if p else "-/%s"
                rows.append("%s | %s | %s | %s | %s | %s | %s | %s" % (
                    name, os.path.basename(nw), "parent only" if p else "new", side % x[1], side % x[2], side % x[3],
                    side % occ(x[3]), side % len(x[0])))
    print("# kernels compared: %d, identical: %d, different: %d, in one build only: %d" % (same + diff, same, diff, only))
    print("kernel | unit | identical | scratch p/n | LDS p/n | VGPR p/n | occ p/n | instr p/n")
    print("\n".join(rows))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
