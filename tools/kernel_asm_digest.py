#!/usr/bin/env python3
"""One line per HIP source: SHA-1 of its gfx950 device assembly (build_hip's flags + --cuda-device-only -S, without the lines
that name the file, the compiler or the source-text hash __hip_cuid_*) and its number of kernels.  Two trees whose lines are
equal build the same GPU code.
usage: tools/kernel_asm_digest.py [--keep DIR]      (--keep also writes the filtered assembly of every source to DIR)"""
import hashlib
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from sunvolumerender_amd import _build  # noqa: E402

keep = Path(sys.argv[sys.argv.index("--keep") + 1]) if "--keep" in sys.argv else None
if keep:
    keep.mkdir(parents=True, exist_ok=True)


def digest(name):
    flags = _build.HIPCC_FLAGS if name not in _build.FAST_SOURCES else [f for f in _build.HIPCC_FLAGS if f not in _build.CONTRACT_FLAGS] + _build.FAST_FLAGS
    res = subprocess.run([_build._hipcc(), *flags, "--cuda-device-only", "-S", str(_build.CSRC / name), "-o", "-"], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed on {name}:\n{res.stderr}")
    for w in (ln for ln in res.stderr.splitlines() if "warning:" in ln and "--hip-link" not in ln):
        print(f"{name}: {w}", file=sys.stderr)
    lines = [ln for ln in res.stdout.splitlines() if not any(k in ln for k in (".file", ".ident", "__hip_cuid_"))]
    text = "\n".join(lines) + "\n"
    if keep:
        (keep / (Path(name).stem + ".s")).write_text(text)
    return f"{name:28s} {hashlib.sha1(text.encode()).hexdigest()}  kernels {sum(ln.lstrip().startswith('.amdhsa_kernel ') for ln in lines):3d}  lines {len(lines)}"


with ThreadPoolExecutor(max_workers=16) as pool:
    for row in pool.map(digest, _build.HIP_SOURCES):
        print(row)
