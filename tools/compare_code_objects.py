#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libbitdelta_hip.so kernel by kernel: same set of functions? same machine code? same address?
Two builds whose kernels are byte-identical can still differ in the ORDER of the kernels in the code object (the order in which the host code
requests the instantiations), and that order alone was worth 0.9 % of the decode step (profiles/decode_dispatch_refactor.txt).  No GPU needed.
usage: python tools/compare_code_objects.py A/libbitdelta_hip.so B/libbitdelta_hip.so"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name, *args):
    return subprocess.check_output([os.path.join(LLVM, name), *args], text=True)


def functions(lib, tmp, tag):
    """name -> (address in the code object, machine code bytes)"""
    fat, co, text = (os.path.join(tmp, f"{tag}.{ext}") for ext in ("fatbin", "co", "text"))
    tool("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat)
    tool("clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}", "--unbundle")
    tool("llvm-objcopy", "-O", "binary", "--only-section=.text", co, text)
    vma = int(re.search(r"\.text\s+PROGBITS\s+([0-9a-f]+)", tool("llvm-readelf", "-SW", co)).group(1), 16)
    code = open(text, "rb").read()
    out = {}
    for line in tool("llvm-readelf", "-sW", co).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            addr, size = int(f[1], 16), int(f[2])
            out[f[7]] = (addr, code[addr - vma:addr - vma + size])
    return out


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        a, b = functions(sys.argv[1], tmp, "a"), functions(sys.argv[2], tmp, "b")
    both = sorted(set(a) & set(b))
    print(f"functions: {len(a)} / {len(b)}, in both {len(both)}, only in the first {len(set(a) - set(b))}, only in the second {len(set(b) - set(a))}")
    print(f"identical machine code: {sum(a[k][1] == b[k][1] for k in both)} of {len(both)}; at another address: {sum(a[k][0] != b[k][0] for k in both)}")
