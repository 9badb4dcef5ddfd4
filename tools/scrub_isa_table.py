#!/usr/bin/env python3
"""The per-kernel resource table of rs_scrub_kernels.hip (profiles/scrub/isa.txt) from the unit's
gfx950 assembly:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/rs_scrub_kernels.hip -o scrub.s
    python3 tools/scrub_isa_table.py scrub.s > profiles/scrub/isa.txt

Another unit's kernels with the same template parameters <K, MT, WPS, UA> are named as the second
argument (profiles/mixed_verify/isa.txt):

    python3 tools/scrub_isa_table.py mixed_fused.s rs_mixed_fused_kernel > profiles/mixed_verify/isa.txt

Reads the .amdhsa_* directives of every kernel descriptor.  Waves per SIMD is what the unified
register file of 512 registers per lane allows (VGPRs and AGPRs, allocated in blocks of 8) capped
at 8, and what the workgroup's LDS allows of the CU's 160 KiB (4 waves per workgroup, one per
SIMD).  Exits non-zero if any kernel uses scratch memory."""
import re
import sys


def main(path, kernel="rs_scrub_mfma_kernel"):
    with open(path) as f:
        src = f.read()
    rows = []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", src, re.S):
        name, body = m.group(1), m.group(2)

        def val(key):
            x = re.search(r"\.amdhsa_%s (\S+)" % key, body)
            return int(x.group(1), 0) if x else 0

        t = re.search(re.escape(kernel) + r"ILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", name)
        if not t:
            continue
        K, MT, WPS, UA = (int(x) for x in t.groups())
        total = val("next_free_vgpr")
        arch = val("accum_offset")
        lds = val("group_segment_fixed_size")
        scratch = val("private_segment_fixed_size")
        alloc = (total + 7) // 8 * 8
        by_reg = min(8, 512 // alloc)
        by_lds = (160 * 1024) // lds if lds else 8
        arch = min(arch, total)  # the offset is rounded up to 4: a kernel without AGPRs
        rows.append((K, MT, UA, WPS, arch, total - arch, total, val("next_free_sgpr"), lds, scratch, min(by_reg, by_lds)))
    rows.sort()
    print("%s<K, MT, WPS, UA>, gfx950: registers per lane, LDS bytes per workgroup, scratch bytes" % kernel)
    print("%3s %3s %-8s %4s %6s %6s %6s %6s %7s %8s %10s" %
          ("K", "MT", "layout", "WPS", "VGPRs", "AGPRs", "total", "SGPRs", "LDS", "scratch", "waves/SIMD"))
    for K, MT, UA, WPS, arch, acc, total, sgpr, lds, scratch, waves in rows:
        print("%3d %3d %-8s %4d %6d %6d %6d %6d %7d %8d %10d" %
              (K, MT, "UA" if UA else "aligned", WPS, arch, acc, total, sgpr, lds, scratch, waves))
    spill = [r for r in rows if r[9]]
    print("%d kernels, %d with scratch" % (len(rows), len(spill)))
    return 1 if spill or not rows else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
