#!/usr/bin/env python3
"""Kernel inventory of the HIP sources: one line per gfx950 kernel with its register, spill,
scratch, LDS, occupancy and code-size figures, for comparing two source trees kernel by kernel.

  python tools/kernel_inventory.py [csrc dir] > listing.txt

Every .hip file is compiled device-only with the Makefile's flags and
-Rpass-analysis=kernel-resource-usage; the code length is the kernel symbol's size in the code
object.  Lines are sorted by (file, demangled name), so `diff` of two listings shows exactly the
kernels that were added, removed or compiled differently."""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
CXXFILT = shutil.which("c++filt") or os.path.join(LLVM, "llvm-cxxfilt")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-fopenmp", "--offload-arch=gfx950", "--offload-device-only",
         "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage", "-c"]
FIELDS = [("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("SGPRs Spill", "sgpr_spill"), ("VGPRs Spill", "vgpr_spill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "lds"),
          ("Occupancy [waves/SIMD]", "occupancy")]


def inventory(path):
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "k.co")
        r = subprocess.run([HIPCC, *FLAGS, path, "-o", co], capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], capture_output=True,
                              text=True, check=True).stdout
    size, kernels = {}, set()
    for ln in syms.splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
        elif len(f) == 8 and f[7].endswith(".kd"):
            kernels.add(f[7][:-3])
    usage, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+(?:Function Name: (\S+)|([A-Za-z][^:]*): (\S+)) \[-Rpass", ln)
        if not m:
            continue
        if m.group(1):
            cur = usage.setdefault(m.group(1), {})
        elif cur is not None:
            cur[m.group(2).strip()] = m.group(3)
    names = sorted(kernels)
    dem = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True,
                         text=True, check=True).stdout.splitlines()
    out = []
    for mangled, name in zip(names, dem):
        u = usage[mangled]
        figs = " ".join(f"{short}={u[key]}" for key, short in FIELDS)
        out.append(f"{os.path.basename(path)} {name.replace(' ', '')} {figs} code_bytes={size[mangled]}")
    return sorted(out)


def main():
    d = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..",
                                                           "python-p2p-network_amd", "csrc")
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=len(files)) as ex:
        for lines in ex.map(inventory, files):
            print("\n".join(lines))


if __name__ == "__main__":
    main()
