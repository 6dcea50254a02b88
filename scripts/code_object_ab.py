#!/usr/bin/env python3
"""Two device-only builds of one translation unit, compared kernel by kernel (developer tool; no GPU):

    hipcc <the build's flags> -DCPPF_BUILD_ID='"x"' --cuda-device-only -c -o a.o cppflow_hip.hip     (once per tree)
    python scripts/code_object_ab.py a.o b.o

A host-only edit can move the order in which kernels are instantiated and with it the bytes of the whole code object, so whole-file
identity is the wrong question.  This unbundles the gfx950 entry of each file and asks, by symbol name: the same set of FUNC symbols;
the same size and code bytes under each name; the same per-kernel entry in the AMDGPU metadata note (registers, LDS, scratch, kernarg
size, argument layout).  Exits non-zero on any difference."""

import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def load(path: str, td: str):
    co = os.path.join(td, os.path.basename(path) + f".{len(os.listdir(td))}.co")
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={path}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)  # fmt: skip
    run = lambda *a: subprocess.run([f"{LLVM}/llvm-readelf", *a, co], capture_output=True, text=True, check=True).stdout
    sections = {}
    for ln in run("-SW").splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", ln)
        if m:
            sections[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16))  # address, file offset
    data = open(co, "rb").read()
    code = {}
    for ln in run("-sW").splitlines():
        f = ln.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6].isdigit():
            addr, off = sections[f[6]]
            at = int(f[1], 16) - addr + off
            code[f[7]] = (int(f[2]), hashlib.sha256(data[at : at + int(f[2])]).hexdigest())
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count", run("--notes"))[1:]:
        blk = blk.split("amdhsa.target")[0]
        meta[re.search(r"\.name:\s+(\S+)", blk).group(1)] = " ".join(blk.split())
    return code, meta


def main() -> int:
    with tempfile.TemporaryDirectory() as td:
        (code_a, meta_a), (code_b, meta_b) = load(sys.argv[1], td), load(sys.argv[2], td)
    bad = 0
    for what, a, b in (("FUNC symbols (size, code bytes)", code_a, code_b), ("kernel metadata entries", meta_a, meta_b)):
        only = sorted(set(a) ^ set(b))
        differ = sorted(k for k in a if k in b and a[k] != b[k])
        print(f"{what}: {len(a)} / {len(b)}, names in one file only: {len(only)}, same name but different: {len(differ)}")
        for k in (only + differ)[:10]:
            print("   ", k)
        bad += len(only) + len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
