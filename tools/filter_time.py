#!/usr/bin/env python3
"""Time the volume filters (svr_volume_rank, svr_volume_smooth) on the phantom head of c3 (512^3).  Per row the HIP-event time of the
call's device work (svr_volume_filter_last_ms: the launches, without the hipMalloc / hipFree of the temporary volume), median of 5 calls
after a warm-up, the time per pass (a rank iteration, or a smoothing axis with a radius > 0), a checksum of the result, and the pass
against two yardsticks:
  the byte floor of a pass -- 4 B per voxel, 2 read and 2 written -- at 8 TB/s (the HBM rate of DESIGN.md section 6), and
  svr_region_apply on the same volume with the bone window's mask, which moves the same bytes (plus the mask): re-measured in the same
  run, as the wall time of batches of 10 calls with one synchronisation per batch, the way tools/region_time.py measures it.
Cases: median / min / max at element 6 / 18 / 26, one iteration; median-26 at 4 iterations; smoothing at radii (1, 1, 1), (2, 2, 2),
(8, 8, 8) and (2, 2, 0).
Every (size, library) pair runs in a child process of its own under its own time limit, so one that goes wrong ends alone.  An A/B build
is named by --lib (a library built with SVR_HIP_LIB=<path> SVR_EXTRA_HIPCC_FLAGS=-D... python -m sunvolumerender_amd._build); the
checksums of the two must agree.
usage: tools/filter_time.py [--n 512] [--lib name=path ...] [--limit SECONDS]"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM = 8e12                                               # bytes / s
OPS = (("median", 1), ("min", 2), ("max", 3))
RADII = ((1, 1, 1), (2, 2, 2), (8, 8, 8), (2, 2, 0))


def child(n: int, tag: str):
    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    vox, _ = scenes._volume("head", n)                  # the c3 (512) phantom, without its gradient pass
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    voxels = vox.size
    words = host.region_mask_words(shape)
    d_vox, d_out, d_mask = dev.malloc(vox.nbytes), dev.malloc(vox.nbytes), dev.malloc(4 * words)
    dev.to_device(d_vox, vox)
    ms = C.c_float()
    floor = 4 * voxels / HBM * 1e3

    def timed(call, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            dev.check(lib.svr_volume_filter_last_ms(C.byref(ms)))
            t.append(ms.value)
        return statistics.median(t), min(t), max(t)

    def crc():
        return zlib.crc32(dev.to_host(d_out, (voxels,), np.uint16).tobytes())

    # the yardstick: svr_region_apply with the bone window's mask
    dev.check(lib.svr_region_threshold(C.c_void_p(d_vox), n, n, n, 1, 39321, 65535, None, None, C.c_void_p(d_mask)))
    dev.synchronize()

    def apply():
        dev.check(lib.svr_region_apply(C.c_void_p(d_vox), n, n, n, 1, C.c_void_p(d_mask), abi.REGION_KEEP, 0, C.c_void_p(d_out)))

    apply()
    dev.synchronize()
    batches = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(10):
            apply()
        dev.synchronize()
        batches.append((time.perf_counter() - t0) / 10 * 1e3)
    ap = statistics.median(batches)
    print(f"{tag} {n}^3: byte floor of a pass {floor:.4f} ms (4 B / voxel at 8 TB/s); svr_region_apply (bone mask) {ap:.3f} ms = {ap / floor:.1f} x floor", flush=True)

    def report(name, t, passes):
        per = t[0] / passes
        print(f"{tag} {n}^3 {name:34s} {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}), {passes} pass(es), {per:7.3f} ms / pass = {per / floor:6.1f} x floor, "
              f"{per / ap:5.1f} x apply, {4 * voxels / (per * 1e-3) / 1e9:7.0f} GB/s, crc {crc():08x}", flush=True)

    for op_name, op in OPS:
        for element in (6, 18, 26):
            t = timed(lambda: dev.check(lib.svr_volume_rank(C.c_void_p(d_vox), n, n, n, 1, op, element, 1, C.c_void_p(d_out))))
            report(f"{op_name} element {element}", t, 1)
    t = timed(lambda: dev.check(lib.svr_volume_rank(C.c_void_p(d_vox), n, n, n, 1, 1, 26, 4, C.c_void_p(d_out))))
    report("median element 26 x 4", t, 4)
    for radii in RADII:
        r = (C.c_uint32 * 3)(*radii)
        t = timed(lambda: dev.check(lib.svr_volume_smooth(C.c_void_p(d_vox), n, n, n, 1, r, C.c_void_p(d_out))))
        report(f"smooth radii {radii}", t, sum(1 for k in radii if k))
    for ptr in (d_vox, d_out, d_mask):
        dev.free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--lib", action="append", default=[], help="name=path of another build to time next to the default one")
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a (size, library) pair may take")
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), a.child[1])
        return 0
    libs = [("default", None)] + [tuple(s.split("=", 1)) for s in a.lib]
    for n in a.n:
        for tag, path in libs:
            env = dict(os.environ)
            if path:
                env["SVR_HIP_LIB"] = str(Path(path).resolve())
            try:
                rc = subprocess.run([sys.executable, __file__, "--child", str(n), tag], env=env, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                print(f"{tag} {n}^3: not finished after {a.limit:.0f} s; stopping here", flush=True)
                return 1
            if rc != 0:
                print(f"{tag} {n}^3: exit status {rc}; stopping here", flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
