#!/usr/bin/env python3
"""Which kernels of a HIP translation unit did a change touch?  Disassembles the gfx950 code objects of two builds of the same object file and
compares every kernel's instruction text (addresses, encodings and the pc-relative literals that hold addresses of data left out).
usage: tools/kernel_diff.py <before.o> <after.o> [name-filter]     e.g. the svr_trace_lm.o of two library builds (sunvolumerender_amd/lib/obj*/)"""
import difflib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/llvm/bin")


def kernels(obj, tmp, tag):
    fb, co = tmp / f"{tag}.fb", tmp / f"{tag}.co"
    cp = tmp / f"{tag}.o"
    cp.write_bytes(Path(obj).read_bytes())          # (objcopy rewrites its input)
    subprocess.run([LLVM / "llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", cp], check=True)
    subprocess.run([LLVM / "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}"], check=True)
    text = subprocess.run([LLVM / "llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            ins = re.sub(r"//.*", "", line).strip()
            if ins:
                cur.append(re.sub(r"(s_addc?_u32 s\d+, s\d+), 0x[0-9a-f]+", r"\1, LIT", ins))
    return out


flt = sys.argv[3] if len(sys.argv) > 3 else ""
with tempfile.TemporaryDirectory() as d:
    a, b = kernels(sys.argv[1], Path(d), "a"), kernels(sys.argv[2], Path(d), "b")
names = subprocess.run(["c++filt"], input="\n".join(a), capture_output=True, text=True).stdout.splitlines()
for k, name in zip(a, names):
    if flt not in name:
        continue
    if k not in b:
        print(f"{name[:110]:110s} {len(a[k]):7d}       - gone")
    elif a[k] == b[k]:
        print(f"{name[:110]:110s} {len(a[k]):7d} {len(b[k]):7d} same")
    else:
        n = sum(1 for x in difflib.unified_diff(a[k], b[k], lineterm="", n=0) if x[0] in "+-" and not x.startswith(("+++", "---")))
        print(f"{name[:110]:110s} {len(a[k]):7d} {len(b[k]):7d} {n} lines differ")
for k in b:
    if k not in a:
        print(f"{k[:110]:110s}       - {len(b[k]):7d} new")
