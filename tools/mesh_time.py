#!/usr/bin/env python3
"""Time the surface-mesh calls (svr_mesh_region, svr_mesh_isosurface, svr_mesh_measure) on the phantom head: the brain and bone window
masks of tools/label_time.py and the raw isosurface at the bone window's lower bound, relax 0 and relax 4 for the masks.  Per case the
HIP-event times of the phases of an EXTRACTION call into buffers of the counted size (svr_mesh_last_ms: classify with the two scans,
emit, relax; the hipMalloc / hipFree of the temporaries, the read-backs of the totals and the bounding-box reduction are outside them),
median of 5 calls after a warm-up with the spread, the vertex and triangle counts, the temporaries in bytes per voxel, and
  (a) the ratio of classify + emit to the byte floor at 8 TB/s (the HBM rate of DESIGN.md section 6): the source read twice (2 B / voxel
      for the volume, 1 bit / voxel for a mask) + the vertices (12 B) and triangles (12 B) written once;
  (b) svr_region_threshold and svr_region_label (connectivity 6) of the same mask from the same job: the neighbouring calls of a chain.
The child process runs under its own time limit.
usage: tools/mesh_time.py [--n 512] [--limit SECONDS]"""
import argparse
import ctypes as C
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM = 8e12                                               # bytes / s


def child(n: int):
    from sunvolumerender_amd import abi, host, scenes

    vox, _ = scenes._volume("head", n)                  # the c3 (512) phantom, without its gradient pass
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    voxels = vox.size
    words = host.region_mask_words(shape)
    d_vox = dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    d_mask, d_labels = dev.malloc(4 * words), dev.malloc(4 * voxels)
    ms = C.c_float()

    def spread(t):
        return f"{statistics.median(t):7.3f} ms ({min(t):.3f} .. {max(t):.3f})"

    def timed_label(call, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            dev.check(lib.svr_region_label_last_ms(C.byref(ms)))
            t.append(ms.value)
        return t

    def mesh_case(name, source_bytes, call, relax):
        info = abi.MeshInfo()
        dev.check(call(None, 0, None, 0, info))
        nv, nt = int(info.vertices), int(info.triangles)
        if nv == 0:
            print(f"{n}^3 {name} relax {relax}: empty mesh", flush=True)
            return
        buf = dev.malloc(12 * (nv + nt))
        phases = [[], [], []]
        for rep in range(6):                             # the first call warms up
            dev.check(call(C.c_void_p(buf), nv, C.c_void_p(buf + 12 * nv), nt, info))
            if rep:
                for k, t in enumerate(dev.mesh_last_ms()):
                    phases[k].append(t)
        both = [a + b for a, b in zip(phases[0], phases[1])]
        floor = (2 * source_bytes + 12 * nv + 12 * nt) / HBM * 1e3
        # the temporaries: one uint64 and two scanned uint32 per wave of 64 padded points; with relax a second vertex array, six links and
        # the cell per vertex
        waves = (shape[0] + 2) * (shape[1] + 2) * ((shape[2] + 2 + 63) // 64)
        temp = 16 * waves * (1 + 1 / 256) + (12 + 28) * nv * (1 if relax else 0)
        print(f"{n}^3 {name} relax {relax}: classify {spread(phases[0])}, emit {spread(phases[1])}, relax {spread(phases[2])}; classify + emit "
              f"{statistics.median(both):.3f} ms = {statistics.median(both) / floor:5.1f} x floor ({floor:.3f} ms); {nv} vertices, {nt} triangles, "
              f"temporaries {temp / voxels:.3f} B / voxel", flush=True)
        scale = (C.c_double * 3)(1 / 256, 1 / 256, 1 / 256)
        vol, area = C.c_int64(), C.c_double()
        dev.check(lib.svr_mesh_measure(C.c_void_p(buf), nv, C.c_void_p(buf + 12 * nv), nt, scale, C.byref(vol), C.byref(area)))
        print(f"{n}^3 {name} relax {relax}: encloses {vol.value / (6 * 256 ** 3):.1f} voxels, area {area.value:.1f} voxel faces", flush=True)
        dev.free(buf)

    cases = [("brain", 23593, 28835), ("bone", 39321, 65535)]
    for name, lo, hi in cases:
        t = timed_label(lambda: dev.check(lib.svr_region_threshold(C.c_void_p(d_vox), n, n, n, 1, lo, hi, None, None, C.c_void_p(d_mask))))
        set_voxels = int(dev.region_stats_of(d_vox, d_mask, shape=shape).voxels)
        print(f"{n}^3 {name} svr_region_threshold {lo}..{hi}: {spread(t)}, {set_voxels} voxels", flush=True)
        k = C.c_uint32()
        t = timed_label(lambda: dev.check(lib.svr_region_label(C.c_void_p(d_mask), n, n, n, 6, C.c_void_p(d_labels), C.byref(k))))
        print(f"{n}^3 {name} svr_region_label conn 6: {spread(t)}, K {k.value}", flush=True)
        for relax in (0, 4):
            p = dev.mesh_params(None, relax)
            mesh_case(name + " mask", voxels / 8,
                      lambda v, nv, tr, nt, info: lib.svr_mesh_region(C.c_void_p(d_mask), n, n, n, C.byref(p), v, nv, tr, nt, C.byref(info)), relax)
    p = dev.mesh_params(cases[1][1], 0)
    mesh_case(f"isosurface at {cases[1][1]}", 2 * voxels,
              lambda v, nv, tr, nt, info: lib.svr_mesh_isosurface(C.c_void_p(d_vox), n, n, n, 1, C.byref(p), v, nv, tr, nt, C.byref(info)), 0)
    for ptr in (d_vox, d_mask, d_labels):
        dev.free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a size may take")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child))
        return 0
    for n in a.n:
        try:
            rc = subprocess.run([sys.executable, __file__, "--child", str(n)], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{n}^3: not finished after {a.limit:.0f} s; stopping here", flush=True)
            return 1
        if rc != 0:
            print(f"{n}^3: exit status {rc}; stopping here", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
