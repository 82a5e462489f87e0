#!/usr/bin/env python3
"""Time the region calls (svr_region_grow, svr_region_stats_of, svr_region_apply) on the phantom head: the brain, bone, air and
whole-volume windows.  Per case: the HIP-event times of classify, grow and stats inside svr_region_grow (svr_region_last_ms), the wall
time of the whole call, of svr_region_stats_of and of svr_region_apply (batches of 10, one synchronisation per batch), the sweep count,
and the fraction of the floor each pass reaches -- the bytes that must move (classify: the u16 volume + two masks written; stats: the
mask + the region's voxels; apply: the volume read and written + the mask) at 8 TB/s, the HBM rate of DESIGN.md section 6.
Medians of 5 calls after a warm-up.  Every (size, library) pair runs in a child process of its own under its own time limit, so one
that goes wrong ends alone; the A/B builds are named by --lib (a library built with SVR_HIP_LIB=<path> SVR_EXTRA_HIPCC_FLAGS=-D...
python -m sunvolumerender_amd._build, e.g. -DSVR_REGION_ALL_TILES: every tile every sweep; -DSVR_REGION_BATCH=1: read the counter every
sweep).
usage: tools/region_time.py [--n 512 [1024]] [--lib name=path ...] [--limit SECONDS]"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM = 8e12                                               # bytes / s


def child(n: int, tag: str):
    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    vox, _ = scenes._volume("head", n)                  # the c3 (512) / c5 (1024) phantom, without its gradient pass
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    words = host.region_mask_words(shape)
    d_vox, d_out, d_mask = dev.malloc(vox.nbytes), dev.malloc(vox.nbytes), dev.malloc(4 * words)
    dev.to_device(d_vox, vox)
    s = n / 48.0                                         # the tests' tiny_head cases, scaled
    bone = np.argwhere(vox[n // 2] >= 39321)[0]
    cases = [("brain", 23593, 28835, (n // 2, n // 2, n // 2)), ("bone", 39321, 65535, (int(bone[1]), int(bone[0]), n // 2)),
             ("air", 0, 0, (0, 0, 0)), ("whole", 0, 65535, (int(7 * s), int(8 * s), int(9 * s)))]
    vol_bytes, mask_bytes = vox.nbytes, 4 * words

    def wall(call, batches=5, reps=10):
        call(); dev.synchronize()
        ms = []
        for _ in range(batches):
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            dev.synchronize()
            ms.append((time.perf_counter() - t0) / reps * 1e3)
        return statistics.median(ms)

    for name, lo, hi, seed in cases:
        p = dev.region_params(lo, hi, 6)
        xyz = (C.c_int32 * 3)(*seed)
        st = abi.RegionStats()

        def grow():
            dev.check(lib.svr_region_grow(C.c_void_p(d_vox), n, n, n, 1, xyz, 1, C.byref(p), C.c_void_p(d_mask), C.byref(st)))

        grow()
        phases, calls = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            grow()
            calls.append((time.perf_counter() - t0) * 1e3)
            ms = [C.c_float(), C.c_float(), C.c_float()]
            lib.svr_region_last_ms(*[C.byref(m) for m in ms])
            phases.append([m.value for m in ms])
        cl, gr, stt = (statistics.median(ph[i] for ph in phases) for i in range(3))
        voxels, sweeps = st.voxels, st.sweeps
        so = wall(lambda: dev.check(lib.svr_region_stats_of(C.c_void_p(d_vox), n, n, n, 1, C.c_void_p(d_mask), C.byref(st))), reps=1)
        ap = wall(lambda: dev.check(lib.svr_region_apply(C.c_void_p(d_vox), n, n, n, 1, C.c_void_p(d_mask), abi.REGION_KEEP, 0, C.c_void_p(d_out))))
        ap_alias = wall(lambda: dev.check(lib.svr_region_apply(C.c_void_p(d_out), n, n, n, 1, C.c_void_p(d_mask), abi.REGION_KEEP, 0, C.c_void_p(d_out))))
        floor_cl = (vol_bytes + 2 * mask_bytes) / HBM * 1e3
        floor_st = (mask_bytes + 2 * voxels) / HBM * 1e3
        floor_ap = (2 * vol_bytes + mask_bytes) / HBM * 1e3
        print(f"{tag} {n}^3 {name:5s} {lo:5d}..{hi:5d}: {voxels:10d} voxels, {sweeps:4d} sweeps | classify {cl:7.3f} ms ({floor_cl / cl:4.2f} of floor)"
              f" grow {gr:8.3f} ms stats {stt:7.3f} ms ({floor_st / stt:4.2f}) | call {statistics.median(calls):8.3f} ms | stats_of call {so:7.3f} ms |"
              f" apply {ap:7.3f} ms ({floor_ap / ap:4.2f}), in place {ap_alias:7.3f} ms", flush=True)
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
