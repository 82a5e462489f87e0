#!/usr/bin/env python3
"""Time the geodesic calls (svr_region_geodesic, svr_region_split) on the phantom head: the brain and bone windows of
tools/distance_time.py.  Per row the HIP-event time of the call's device work (svr_region_geodesic_last_ms: the launches, without the
hipMalloc / hipFree of the workspace), median of 3 calls after a warm-up, the sweeps launched, and a checksum of the result:
  svr_region_geodesic from ONE seed (the voxel of the mask nearest its centroid) under the chamfer weights, and from the CORES of the
    mask -- what a ball of 2 mm leaves at spacing 0.7, 0.7, 1.5, labelled under connectivity 26 -- under the weights of
    svr_region_geodesic_weights;
  svr_region_split with the same ball, phase by phase: erode (svr_region_distance_last_ms), label (svr_region_label_last_ms), zones
    (svr_region_geodesic_last_ms);
  for comparison svr_region_reconstruct (connectivity 26) with the same markers and domain: the binary form of the same propagation on the
    same kind of sweeps, so the floor this kernel can approach.  The ratio of the two times and the sweeps of both are printed.
  The byte floor at 8 TB/s (the HBM rate of DESIGN.md section 6) counts what init and finish alone must move: the labels and the mask
    read, 8 B of key written and read, the outputs written.
Every size runs in a child process under its own time limit, so one that goes wrong ends alone.  The lines go to stdout and to --out.
usage: tools/geodesic_time.py [--n 512] [--limit SECONDS] [--out profiles/geodesic_times.txt]"""
import argparse
import ctypes as C
import statistics
import subprocess
import sys
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM = 8e12                                               # bytes / s
SPACING = (0.7, 0.7, 1.5)
CORE_RADIUS = 2.0                                        # mm
REPS = 3


def child(n: int, out: str):
    import builtins

    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    def print(*args, **kw):                             # every line goes to stdout and to the record
        builtins.print(*args, **kw)
        with open(out, "a") as f:
            builtins.print(*args, file=f)

    vox, _ = scenes._volume("head", n)                  # the c3 (512) phantom, without its gradient pass
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    voxels = vox.size
    words = host.region_mask_words(shape)
    d_vox = dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    d_mask, d_cores, d_out = (dev.malloc(4 * words) for _ in range(3))
    d_labels, d_dist, d_zones = (dev.malloc(4 * voxels) for _ in range(3))
    ms = C.c_float()

    def last(fn):
        dev.check(fn(C.byref(ms)))
        return ms.value

    def timed(call, last_ms):
        call()
        t = []
        for _ in range(REPS):
            call()
            t.append(last(last_ms))
        return statistics.median(t), min(t), max(t)

    def crc(ptr, count):
        return zlib.crc32(dev.to_host(ptr, (count,), np.uint32).tobytes())

    dw, unit = host.distance_weights(SPACING, shape)
    steps, step_unit = host.geodesic_weights(SPACING, 26, shape)
    r2 = int((CORE_RADIUS / unit) ** 2)
    cdw, csteps = (C.c_uint32 * 3)(*dw), (C.c_uint32 * 7)(*steps)
    floor_b = 4 + 1 / 8 + 8 + 8 + 4 + 4                                  # bytes per voxel: labels, mask, keys out and in, dist, zones
    floor = floor_b * voxels / HBM * 1e3
    print(f"{n}^3: distance weights {dw} unit {unit:g}, step weights {steps} unit {step_unit:g}, core r2 {r2}; byte floor {floor_b:.1f} B / voxel = {floor:.3f} ms",
          flush=True)
    sweeps = C.c_uint32()
    for name, lo, hi in (("brain", 23593, 28835), ("bone", 39321, 65535)):
        dev.check(lib.svr_region_threshold(C.c_void_p(d_vox), n, n, n, 1, lo, hi, None, None, C.c_void_p(d_mask)))
        dev.synchronize()
        mask = host.region_mask_unpack(dev.to_host(d_mask, (words,), np.uint32), shape)
        at = np.argwhere(mask)
        seed = at[np.argmin(((at - at.mean(axis=0)) ** 2).sum(axis=1))][::-1]             # (x, y, z)
        print(f"{n}^3 {name}: {int(mask.sum())} voxels, seed {tuple(int(t) for t in seed)}", flush=True)
        # the cores: erode by the ball, label
        dev.check(lib.svr_region_ball(C.c_void_p(d_mask), n, n, n, abi.MORPH_ERODE, cdw, r2, C.c_void_p(d_cores)))
        for mname, weights in (("one seed, chamfer", None), ("cores, spacing", csteps)):
            if weights is None:
                dev.region_seed_labels([seed], shape, out_ptr=d_labels)
                marker = np.zeros(words, dtype=np.uint32)
                wx = (shape[2] + 31) // 32
                marker[(int(seed[2]) * shape[1] + int(seed[1])) * wx + int(seed[0]) // 32] = 1 << (int(seed[0]) % 32)
                dev.to_device(d_out, marker)
                d_marker, cores = d_out, 1
            else:
                k = C.c_uint32()
                dev.check(lib.svr_region_label(C.c_void_p(d_cores), n, n, n, 26, C.c_void_p(d_labels), C.byref(k)))
                d_marker, cores = d_cores, int(k.value)
            t = timed(lambda: dev.check(lib.svr_region_geodesic(C.c_void_p(d_labels), C.c_void_p(d_mask), n, n, n, weights, 0, C.c_void_p(d_dist),
                                                                C.c_void_p(d_zones), C.byref(sweeps))), lib.svr_region_geodesic_last_ms)
            gs = int(sweeps.value)
            d = dev.to_host(d_dist, shape, np.uint32)
            reached = d != abi.GEO_NONE
            line = (f"{n}^3 {name:5s} geodesic {mname} ({cores} markers): {t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; {t[0] / floor:7.1f} x byte floor), {gs} sweeps, "
                    f"{int(reached.sum())} reached, max dist {int(d[reached].max()) if reached.any() else 0}, crc {crc(d_dist, voxels):08x} {crc(d_zones, voxels):08x}")
            print(line, flush=True)
            d_rec = dev.malloc(4 * words)
            r = timed(lambda: dev.check(lib.svr_region_reconstruct(C.c_void_p(d_marker), C.c_void_p(d_mask), n, n, n, 26, 0, C.c_void_p(d_rec), C.byref(sweeps))),
                      lib.svr_region_mask_last_ms)
            rec = host.region_mask_unpack(dev.to_host(d_rec, (words,), np.uint32), shape)
            dev.free(d_rec)
            print(f"{n}^3 {name:5s} reconstruct {mname}: {r[0]:9.3f} ms ({r[1]:.3f} .. {r[2]:.3f}), {int(sweeps.value)} sweeps, {int(rec.sum())} voxels "
                  f"(equal to the reached set: {bool(np.array_equal(rec, reached))}); geodesic / reconstruct = {t[0] / r[0]:.1f} x in time, "
                  f"{gs / max(int(sweeps.value), 1):.2f} x in sweeps", flush=True)
        count, lost = C.c_uint32(), C.c_uint32()
        phases = []
        for _ in range(REPS + 1):
            dev.check(lib.svr_region_split(C.c_void_p(d_mask), n, n, n, cdw, r2, 26, csteps, 0, C.c_void_p(d_zones), C.byref(count), C.byref(lost), C.byref(sweeps)))
            phases.append((last(lib.svr_region_distance_last_ms), last(lib.svr_region_label_last_ms), last(lib.svr_region_geodesic_last_ms)))
        e, l, z = (statistics.median(p[i] for p in phases[1:]) for i in range(3))
        print(f"{n}^3 {name:5s} split r2 {r2} conn 26: erode {e:.3f} ms, label {l:.3f} ms, zones {z:.3f} ms ({int(sweeps.value)} sweeps); {int(count.value)} parts, "
              f"{int(lost.value)} voxels unreached, crc {crc(d_zones, voxels):08x}", flush=True)
        t = timed(lambda: dev.check(lib.svr_region_zone_cut(C.c_void_p(d_zones), n, n, n, 26, C.c_void_p(d_out))), lib.svr_region_geodesic_last_ms)
        print(f"{n}^3 {name:5s} zone_cut conn 26: {t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f}), crc {crc(d_out, words):08x}", flush=True)
    for ptr in (d_vox, d_mask, d_cores, d_out, d_labels, d_dist, d_zones):
        dev.free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--limit", type=float, default=400.0, help="seconds a size may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "geodesic_times.txt"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child), a.out)
        return 0
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("")
    for n in a.n:
        try:
            rc = subprocess.run([sys.executable, __file__, "--child", str(n), "--out", a.out], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = None
        if rc != 0:
            line = f"{n}^3: " + (f"not finished after {a.limit:.0f} s" if rc is None else f"exit status {rc}") + "; stopping here"
            print(line, flush=True)
            with open(a.out, "a") as f:
                print(line, file=f)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
