#!/usr/bin/env python3
"""Registers, scratch, LDS and instruction count of the kernels of a built libdfx.so whose names match a pattern, one JSON line
per kernel (no GPU needed): the code objects are taken out of the library with the method of
tests/test_farneback_kernel_resources.py, the figures read from their metadata notes, and the instructions counted as the lines
of llvm-objdump's disassembly between a kernel's label and the next.

    scripts/kernel_resources.py LIB [REGEX]        e.g.  'k_fb_check|k_warp|k_flow_chain|k_gm_|k_fp_|k_flow_median|k_interp|k_flowvis|merge_planar'
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
FIELDS = r"\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_count):\s+(\d+)"


def tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else shutil.which(name)


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    lib, pattern = sys.argv[1], re.compile(sys.argv[2] if len(sys.argv) > 2 else ".")
    objcopy, bundler, readelf, objdump, filt = (tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf",
                                                                   "llvm-objdump", "llvm-cxxfilt"))
    rows = {}
    with tempfile.TemporaryDirectory() as d:
        fatbin = os.path.join(d, "lib.fatbin")
        subprocess.run([objcopy, "-O", "binary", "--only-section=.hip_fatbin", lib, fatbin], check=True)
        with open(fatbin, "rb") as f:
            data = f.read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
        for i, s in enumerate(starts):  # one offload bundle per translation unit, back to back
            part, co = os.path.join(d, f"b{i}.bundle"), os.path.join(d, f"b{i}.co")
            with open(part, "wb") as f:
                f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
            subprocess.run([bundler, "--type=o", "--unbundle", f"--input={part}", f"--output={co}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
            notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"\n\s*- \.", notes):
                name = re.search(r"\.name:\s+(\S+)", block)
                if name and pattern.search(name.group(1)):
                    rows[name.group(1)] = {k: int(v) for k, v in re.findall(FIELDS, block)}
            label, count = None, 0
            for line in subprocess.run([objdump, "-d", co], check=True, capture_output=True, text=True).stdout.splitlines():
                m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
                if m:
                    if label in rows:
                        rows[label]["instructions"] = count
                    label, count = m.group(1), 0
                elif re.match(r"\s+\S+.*//", line):
                    count += 1
            if label in rows:
                rows[label]["instructions"] = count
    names = subprocess.run([filt or "c++filt"], input="\n".join(rows), capture_output=True, text=True, check=True).stdout.splitlines()
    for mangled, nice in sorted(zip(rows, names), key=lambda p: p[1]):
        r = rows[mangled]
        nice = re.sub(r"\(anonymous namespace\)::|^void ", "", nice).split("(")[0]
        print(json.dumps(dict(kernel=nice, vgpr=r["vgpr_count"], scratch=r["private_segment_fixed_size"],
                              lds=r["group_segment_fixed_size"], instructions=r.get("instructions"))))


if __name__ == "__main__":
    main()
