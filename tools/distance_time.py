#!/usr/bin/env python3
"""Time the distance calls (svr_region_distance, svr_region_ball, svr_region_distance_max) on the phantom head: the brain and bone
windows of tools/region_time.py.  Per row the HIP-event time of the call's device work (svr_region_distance_last_ms: the launches,
without the hipMalloc / hipFree of the workspace), median of 5 calls after a warm-up, a checksum of the result, and
  the per-pass split of the last transform (svr_region_distance_pass_ms: rows, y, z),
  the bytes the passes move -- rows: the mask read + 4 B / voxel written; each column pass: 4 B / voxel read, 4 B / voxel written (the
  last pass of a ball: the mask written instead) and up to 4 B / voxel of stack written and read -- and
  the ratio of the time to the byte floor at 8 TB/s (the HBM rate of DESIGN.md section 6): the mask read and the map written once for
  svr_region_distance, two masks for svr_region_ball, the map (and the mask) read for svr_region_distance_max.
Cases: svr_region_distance for both targets under weights (1, 1, 1) and those of svr_region_distance_weights for spacing 0.7, 0.7, 1.5;
svr_region_ball open and close at radii of 1, 8, 32 and 100 voxel units; svr_region_distance_max.  As the yardstick from the same job:
svr_region_morph open and close by 8 under elements 6 and 26 (svr_region_mask_last_ms).
Every (size, library) pair runs in a child process of its own under its own time limit, so one that goes wrong ends alone.  An A/B
build is named by --lib (a library built with SVR_HIP_LIB=<path> SVR_EXTRA_HIPCC_FLAGS=-DSVR_DISTANCE_BRUTE python -m
sunvolumerender_amd._build: the literal O(n^2) per column min-plus passes); it runs at --ab-n (default 128: the brute passes cost n
times as much per voxel), next to the default library at that size, and the checksums of the two must agree.
usage: tools/distance_time.py [--n 512] [--ab-n 128] [--lib name=path ...] [--limit SECONDS]"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM = 8e12                                               # bytes / s
SPACING = (0.7, 0.7, 1.5)
RADII = (1, 8, 32, 100)


def child(n: int, tag: str):
    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    vox, _ = scenes._volume("head", n)                  # the c3 (512) phantom, without its gradient pass
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    voxels = vox.size
    words = host.region_mask_words(shape)
    d_vox = dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    d_mask, d_out, d_map = dev.malloc(4 * words), dev.malloc(4 * words), dev.malloc(4 * voxels)
    ms = C.c_float()

    def timed(call, last_ms, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            dev.check(last_ms(C.byref(ms)))
            t.append(ms.value)
        return statistics.median(t), min(t), max(t)

    def split():
        r, y, z = dev.region_distance_pass_ms()
        return f"rows {r:.3f} y {y:.3f} z {z:.3f} ms"

    def crc(ptr, count):
        return zlib.crc32(dev.to_host(ptr, (count,), np.uint32).tobytes())

    weights = {"w 1 1 1": (1, 1, 1), "w spacing": host.distance_weights(SPACING, shape)[0]}
    unit_w = (C.c_uint32 * 3)(1, 1, 1)
    moved_map = 4 * words + 4 * voxels + 2 * (8 + 8) * voxels            # rows, then two column passes with their stacks (upper bound)
    moved_ball = 4 * words + 4 * voxels + (8 + 8) * voxels + (4 + 8) * voxels + 4 * words
    for name, lo, hi in (("brain", 23593, 28835), ("bone", 39321, 65535)):
        dev.check(lib.svr_region_threshold(C.c_void_p(d_vox), n, n, n, 1, lo, hi, None, None, C.c_void_p(d_mask)))
        dev.synchronize()
        print(f"{tag} {n}^3 {name}: {int(dev.region_stats_of(d_vox, d_mask, shape=shape).voxels)} voxels", flush=True)
        for wname, w in weights.items():
            cw = (C.c_uint32 * 3)(*w)
            for tname, target in (("to_set", abi.DIST_TO_SET), ("to_unset", abi.DIST_TO_UNSET)):
                t = timed(lambda: dev.check(lib.svr_region_distance(C.c_void_p(d_mask), n, n, n, cw, target, C.c_void_p(d_map))),
                          lib.svr_region_distance_last_ms)
                floor = (4 * words + 4 * voxels) / HBM * 1e3
                print(f"{tag} {n}^3 {name:5s} distance {tname:8s} {wname} {w}: {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; {t[0] / floor:6.1f} x floor "
                      f"{floor:.3f} ms; moves <= {moved_map / 1e6:.0f} MB = {moved_map / HBM * 1e3:.3f} ms), {split()}, crc {crc(d_map, voxels):08x}", flush=True)
        # (d_map: the TO_UNSET map under the spacing's weights)
        m, first, status = C.c_uint32(), C.c_uint32(), C.c_int32()
        for mname, mask in (("in the mask", C.c_void_p(d_mask)), ("no mask", None)):
            t = timed(lambda: dev.check(lib.svr_region_distance_max(C.c_void_p(d_map), mask, n, n, n, C.byref(m), C.byref(first), C.byref(status))),
                      lib.svr_region_distance_last_ms)
            floor = (4 * voxels + (4 * words if mask else 0)) / HBM * 1e3
            print(f"{tag} {n}^3 {name:5s} distance_max {mname}: {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; {t[0] / floor:6.1f} x floor), max d2 {m.value} "
                  f"at {first.value}, status {status.value}", flush=True)
        for op_name, op in (("open", abi.MORPH_OPEN), ("close", abi.MORPH_CLOSE)):
            for radius in RADII:
                if radius >= n:
                    continue
                t = timed(lambda: dev.check(lib.svr_region_ball(C.c_void_p(d_mask), n, n, n, op, unit_w, radius * radius, C.c_void_p(d_out))),
                          lib.svr_region_distance_last_ms)
                floor = 2 * 4 * words / HBM * 1e3
                print(f"{tag} {n}^3 {name:5s} ball {op_name:5s} radius {radius:3d}: {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; {t[0] / floor:7.1f} x floor; two transforms "
                      f"move <= {2 * moved_ball / 1e6:.0f} MB = {2 * moved_ball / HBM * 1e3:.3f} ms), second: {split()}, crc {crc(d_out, words):08x}", flush=True)
            for element in (6, 26):                      # the yardstick: the iterated unit element
                t = timed(lambda: dev.check(lib.svr_region_morph(C.c_void_p(d_mask), n, n, n, op, element, 8, C.c_void_p(d_out))), lib.svr_region_mask_last_ms)
                print(f"{tag} {n}^3 {name:5s} morph {op_name:5s} element {element:2d} radius 8: {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}), crc {crc(d_out, words):08x}",
                      flush=True)
    for ptr in (d_vox, d_mask, d_out, d_map):
        dev.free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--ab-n", type=int, default=128, help="the size at which the --lib builds (and the default one next to them) run")
    ap.add_argument("--lib", action="append", default=[], help="name=path of another build to time next to the default one")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a (size, library) pair may take")
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), a.child[1])
        return 0
    runs = [(n, "default", None) for n in a.n]
    if a.lib:
        runs += [(a.ab_n, "default", None)] + [(a.ab_n,) + tuple(s.split("=", 1)) for s in a.lib]
    for n, tag, path in runs:
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
