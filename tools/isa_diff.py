#!/usr/bin/env python3
"""Compare the gfx950 code of two builds kernel by kernel:

    python3 tools/isa_diff.py OLD_BUILD_DIR NEW_BUILD_DIR [unit ...]

For every object file both directories hold (or the named units), the device code object is taken
out of the host object's .hip_fatbin section (llvm-objcopy, clang-offload-bundler), disassembled (llvm-objdump -d) and split at the
function symbols; addresses and encodings are dropped, so two functions are equal when they hold
the same instructions with the same operands.  Prints one line per unit and the count compared;
functions only the new build holds are counted as added, not as differing.  Exits non-zero when a
function differs or only the old build holds it."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def functions(obj, tmp):
    fat, co = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj],
                          stderr=subprocess.DEVNULL)
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET,
                           "--input=" + fat, "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip() and line.strip() != "...":  # "...": the padding objdump elides after a function
            # drop the trailing address comment; branch targets stay symbolic (<name+0x..>)
            out[name].append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def main(old, new, units):
    if not units:
        units = sorted(f for f in os.listdir(old) if f.endswith(".o") and os.path.exists(os.path.join(new, f)))
    total = bad = added = 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            try:
                a, b = functions(os.path.join(old, u), tmp), functions(os.path.join(new, u), tmp)
            except subprocess.CalledProcessError:
                continue  # no device code in this object
            diff = sorted(n for n in a if a[n] != b.get(n))
            more = len(set(b) - set(a))
            total += len(set(a) & set(b))
            bad += len(diff)
            added += more
            print("%-28s %4d functions, %d differ%s%s" % (u, len(set(a) & set(b)), len(diff),
                                                          ", %d added" % more if more else "",
                                                          ": " + ", ".join(diff[:3]) if diff else ""))
    print("%d compared, %d differ%s" % (total, bad, ", %d added" % added if added else ""))
    return 1 if bad or not total else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
