#!/usr/bin/env python3
"""Time the component calls (svr_region_threshold, _label, _label_table, _select_by_size) on the phantom head: the brain, bone and air
windows of tools/region_time.py and the full mask, connectivity 6 and 26.  Per row the HIP-event time of the call's device work
(svr_region_label_last_ms: for svr_region_label everything from the first launch to the last, without the hipMalloc / hipFree of the
temporaries and the read-back of K; for svr_region_select_by_size the read-back of the table and the upload of the keep array included),
median of 5 calls after a warm-up, with K, and the ratio to the byte floor at 8 TB/s (the HBM rate of DESIGN.md section 6):
  label   the label array written once (4 B / voxel) + the mask read 4 times, the root mask and the scan array written and read
  table   the label array read (4 B / voxel) + the volume (2 B / voxel)
  select  the label array read + the mask written
As a yardstick from the same job: svr_region_grow's grow phase on the whole-volume window ("whole" of tools/region_time.py), which
resolves the same connectivity as the full mask on bit masks alone.
Every (size, library) pair runs in a child process of its own under its own time limit, so one that goes wrong ends alone; an A/B build
is named by --lib (a library built with SVR_HIP_LIB=<path> SVR_EXTRA_HIPCC_FLAGS=-D... python -m sunvolumerender_amd._build:
-DSVR_LABEL_GLOBAL_ONLY: every voxel a node, every backward neighbour a union; -DSVR_LABEL_TABLE_PLAIN: every run issues its own
atomics), and the default library is then timed once more after the others, so that the job shows its own run-to-run spread.  Every
build's labels are compared with the first build's by a checksum.
usage: tools/label_time.py [--n 512] [--lib name=path ...] [--limit SECONDS]"""
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
    d_mask, d_out, d_labels = dev.malloc(4 * words), dev.malloc(4 * words), dev.malloc(4 * voxels)
    ms = C.c_float()

    def timed(call, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            dev.check(lib.svr_region_label_last_ms(C.byref(ms)))
            t.append(ms.value)
        return statistics.median(t), min(t), max(t)

    # the yardstick: the grow phase of svr_region_grow on the whole-volume window
    s = n / 48.0
    p = dev.region_params(0, 65535, 6)
    xyz = (C.c_int32 * 3)(int(7 * s), int(8 * s), int(9 * s))
    st = abi.RegionStats()
    phases = []
    for _ in range(6):
        dev.check(lib.svr_region_grow(C.c_void_p(d_vox), n, n, n, 1, xyz, 1, C.byref(p), C.c_void_p(d_out), C.byref(st)))
        g = [C.c_float(), C.c_float(), C.c_float()]
        lib.svr_region_last_ms(*[C.byref(t) for t in g])
        phases.append(g[1].value)
    print(f"{tag} {n}^3 svr_region_grow whole volume conn 6: grow phase {statistics.median(phases[1:]):.3f} ms "
          f"({min(phases[1:]):.3f} .. {max(phases[1:]):.3f}), {st.sweeps} sweeps, {st.voxels} voxels", flush=True)

    cases = [("brain", 23593, 28835), ("bone", 39321, 65535), ("air", 0, 0), ("full", 0, 65535)]
    for name, lo, hi in cases:
        t = timed(lambda: dev.check(lib.svr_region_threshold(C.c_void_p(d_vox), n, n, n, 1, lo, hi, None, None, C.c_void_p(d_mask))))
        floor = (2 * voxels + 4 * words) / HBM * 1e3
        set_voxels = int(dev.region_stats_of(d_vox, d_mask, shape=shape).voxels)
        print(f"{tag} {n}^3 {name:5s} threshold {lo}..{hi}: {t[0]:7.3f} ms ({t[0] / floor:5.1f} x floor), {set_voxels} voxels", flush=True)
        for conn in (6, 26):
            k = C.c_uint32()
            t = timed(lambda: dev.check(lib.svr_region_label(C.c_void_p(d_mask), n, n, n, conn, C.c_void_p(d_labels), C.byref(k))))
            floor = (4 * voxels + 4 * 4 * words + 4 * 4 * words) / HBM * 1e3
            crc = zlib.crc32(dev.to_host(d_labels, (voxels,), np.uint32).tobytes())
            print(f"{tag} {n}^3 {name:5s} conn {conn:2d} label : {t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; {t[0] / floor:5.1f} x floor), K {k.value}, "
                  f"labels crc {crc:08x}", flush=True)
            if k.value == 0:
                continue
            d_table = dev.malloc(40 * k.value)
            for what, src in (("table with sum", C.c_void_p(d_vox)), ("table, no volume", None)):
                t = timed(lambda: dev.check(lib.svr_region_label_table(C.c_void_p(d_labels), src, n, n, n, 1, k.value, C.c_void_p(d_table))))
                floor = (4 + (2 if src else 0)) * voxels / HBM * 1e3
                print(f"{tag} {n}^3 {name:5s} conn {conn:2d} {what:16s}: {t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; {t[0] / floor:5.1f} x floor)", flush=True)
            table = dev.to_host(d_table, (k.value,), host.COMPONENT_DTYPE)
            kept = C.c_uint32()
            for min_voxels, largest_k in ((0, 1), (100, 0)):
                t = timed(lambda: dev.check(lib.svr_region_select_by_size(C.c_void_p(d_labels), n, n, n, k.value, C.c_void_p(d_table), min_voxels,
                                                                          largest_k, C.c_void_p(d_out), C.byref(kept))))
                floor = (4 * voxels + 4 * words) / HBM * 1e3
                left = int(dev.region_stats_of(d_vox, d_out, shape=shape).voxels)
                print(f"{tag} {n}^3 {name:5s} conn {conn:2d} select_by_size min {min_voxels} k {largest_k}: {t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; "
                      f"{t[0] / floor:5.1f} x floor), kept {kept.value} of {k.value}, {left} voxels; largest component {int(table['voxels'].max())}", flush=True)
            dev.free(d_table)
    for ptr in (d_vox, d_mask, d_out, d_labels):
        dev.free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--lib", action="append", default=[], help="name=path of another build to time next to the default one")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a (size, library) pair may take")
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), a.child[1])
        return 0
    libs = [("default", None)] + [tuple(s.split("=", 1)) for s in a.lib] + ([("default-again", None)] if a.lib else [])
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
