#!/usr/bin/env python3
"""Time the smoothing calls (svr_region_box_count, svr_region_smooth, svr_region_label_smooth) on the phantom head with the brain and bone
windows' masks.  HIP-event times, median of 5 calls after a warm-up (min .. max), unless a row says wall clock:
  majority    svr_region_smooth MAJORITY at r = 1, 2, 4, 8, against (a) its byte floor of 8 B per mask word at 8 TB/s, (b)
              svr_region_morph OPEN, element 26, of the same radius, (c) for r = 1 svr_volume_rank MEDIAN 26 on the u16 voxels;
  count       svr_region_box_count at the same radii, against its write floor of 2 B per voxel;
  binomial    svr_region_smooth BINOMIAL against the composition svr_region_apply on a constant 65535 volume, svr_volume_smooth,
              svr_region_threshold; both by the wall clock around the calls and a synchronisation;
  mode        svr_region_label_smooth of three classes that cover the volume (below the brain window, up to the bone window, bone) and
              of the 26-connected parts of the bone mask and the zones of svr_region_split of it (labels above 255 read as background),
              against one pass of the label planes' bytes plus classes x MAJORITY, with the share of tiles whose halo holds one label
              (they are written without counting);
  mesh        svr_mesh_region + svr_mesh_measure before and after MAJORITY r = 1: of the bone mask, and of the largest part of the bone
              window of the voxels with uniform noise of +- 4000 added (a ragged mask).
The size runs in a child process under its own time limit, so one that goes wrong ends alone.
usage: tools/smooth_time.py [--n 512] [--limit SECONDS]"""
import argparse
import ctypes as C
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM = 8e12                                               # bytes / s
TW, TY, TZ = 4, 8, 8                                     # the tile of csrc/svr_smooth.hip in words, rows, slices


def single_label_tiles(labels, r):
    """the share of tiles of csrc/svr_smooth.hip whose halo (one word in x, r rows and slices) holds one label only"""
    import numpy as np

    nz, ny, nx = labels.shape
    wx = (nx + 31) // 32
    pad = np.pad(labels, ((0, 0), (0, 0), (0, wx * 32 - nx)), mode="edge").reshape(nz, ny, wx, 32)
    lo, hi = pad.min(axis=3), pad.max(axis=3)
    one = total = 0
    for z0 in range(0, nz, TZ):
        zs = slice(max(z0 - r, 0), z0 + TZ + r)
        for y0 in range(0, ny, TY):
            ys = slice(max(y0 - r, 0), y0 + TY + r)
            for w0 in range(0, wx, TW):
                ws = slice(max(w0 - 1, 0), w0 + TW + 1)
                total += 1
                one += int(lo[zs, ys, ws].min() == hi[zs, ys, ws].max())
    return one / total


def child(n: int):
    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    vox = scenes.make_scene("c3", n=n).vox               # the c3 phantom (n = 512 is c3 itself)
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    words = host.region_mask_words(shape)
    dims = (C.c_int32 * 3)(n, n, n)
    ms = C.c_float()
    p = lambda ptr: C.c_void_p(ptr)                      # noqa: E731
    u32 = lambda *v: (C.c_uint32 * 3)(*v)                # noqa: E731

    def timed(call, read, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            t.append(read())
        return statistics.median(t), min(t), max(t)

    def wall(call, reps=5):
        def once():
            dev.synchronize()
            t0 = time.perf_counter()
            call()
            dev.synchronize()
            return (time.perf_counter() - t0) * 1e3
        once()
        t = [once() for _ in range(reps)]
        return statistics.median(t), min(t), max(t)

    def last(fn):
        def read():
            dev.check(fn(C.byref(ms)))
            return ms.value
        return read

    def fmt(t):
        return f"{t[0]:8.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"

    smooth_ms, mask_ms, filter_ms = last(lib.svr_region_smooth_last_ms), last(lib.svr_region_mask_last_ms), last(lib.svr_volume_filter_last_ms)
    d_vox, d_u16, d_full = dev.malloc(vox.nbytes), dev.malloc(vox.nbytes), dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    dev.to_device(d_full, np.full(shape, 65535, np.uint16))
    d_mask, d_out = dev.malloc(4 * words), dev.malloc(4 * words)
    d_lab, d_lab_out = dev.malloc(4 * vox.size), dev.malloc(4 * vox.size)
    f_mask, f_count = 8 * words / HBM * 1e3, 2 * vox.size / HBM * 1e3
    t_median = timed(lambda: dev.check(lib.svr_volume_rank(p(d_vox), n, n, n, 1, abi.FILTER_MEDIAN, 26, 1, p(d_u16))), filter_ms)
    print(f"{n}^3: svr_volume_rank MEDIAN 26 on the u16 voxels {fmt(t_median)}; byte floor of a mask pass {f_mask:.5f} ms, of a u16 volume written {f_count:.4f} ms", flush=True)
    majority = {}
    for window, lo, hi in (("brain", 23593, 28835), ("bone", 39321, 65535)):
        dev.check(lib.svr_region_threshold(p(d_vox), n, n, n, 1, lo, hi, None, None, p(d_mask)))
        dev.synchronize()
        mask = host.region_mask_unpack(dev.to_host(d_mask, (words,), np.uint32), shape)
        print(f"{n}^3 {window}: {int(mask.sum())} voxels", flush=True)
        for r in (1, 2, 4, 8):
            changed = C.c_uint64(0)
            dev.check(lib.svr_region_smooth(p(d_mask), dims, abi.SMOOTH_MAJORITY, u32(r, r, r), 1, p(d_out), C.byref(changed)))
            t_maj = timed(lambda: dev.check(lib.svr_region_smooth(p(d_mask), dims, abi.SMOOTH_MAJORITY, u32(r, r, r), 1, p(d_out), None)), smooth_ms)
            t_open = timed(lambda: dev.check(lib.svr_region_morph(p(d_mask), n, n, n, abi.MORPH_OPEN, 26, r, p(d_out))), mask_ms)
            t_count = timed(lambda: dev.check(lib.svr_region_box_count(p(d_mask), dims, u32(r, r, r), p(d_u16))), smooth_ms)
            majority[(window, r)] = t_maj[0]
            print(f"    r = {r}: majority {fmt(t_maj)} = {t_maj[0] / f_mask:6.1f} x floor, {t_maj[0] / t_open[0]:5.2f} x OPEN 26 ({t_open[0]:.4f} ms)"
                  + (f", {t_maj[0] / t_median[0]:5.2f} x MEDIAN 26 on u16" if r == 1 else "") + f"; {changed.value} voxels change", flush=True)
            print(f"           count    {fmt(t_count)} = {t_count[0] / f_count:6.1f} x floor", flush=True)
        for radii in ((1, 1, 1), (2, 2, 2), (8, 8, 8)):
            t_bin = wall(lambda: dev.check(lib.svr_region_smooth(p(d_mask), dims, abi.SMOOTH_BINOMIAL, u32(*radii), 1, p(d_out), None)))

            def composition():
                dev.check(lib.svr_region_apply(p(d_full), n, n, n, 1, p(d_mask), abi.REGION_KEEP, 0, p(d_u16)))
                dev.check(lib.svr_volume_smooth(p(d_u16), n, n, n, 1, u32(*radii), p(d_lab)))          # (d_lab: any buffer of the size)
                dev.check(lib.svr_region_threshold(p(d_lab), n, n, n, 1, 32768, 65535, None, None, p(d_out)))
            t_comp = wall(composition)
            print(f"    binomial {radii}: {fmt(t_bin)} wall clock = {t_bin[0] / t_comp[0]:5.2f} x the three-call composition ({fmt(t_comp)})", flush=True)
    # ---- the mode filter
    three = (1 + (vox >= 23593) + (vox >= 39321)).astype(np.uint32)
    dev.check(lib.svr_region_threshold(p(d_vox), n, n, n, 1, 39321, 65535, None, None, p(d_mask)))
    k = C.c_uint32(0)
    dev.check(lib.svr_region_label(p(d_mask), n, n, n, 26, p(d_lab), C.byref(k)))
    parts = dev.to_host(d_lab, shape, np.uint32)
    parts[parts > 255] = 0
    zones, nzones, _, _ = dev.region_split(d_mask, 16, 26, shape=shape)      # necks thinner than a ball of radius 4 voxels are cut
    zones[zones > 255] = 0
    for name, labels, count in (("three classes over the volume", three, 3), (f"the {k.value} parts of the bone mask (255 kept)", parts, min(int(k.value), 255)),
                                (f"the {nzones} zones of svr_region_split of the bone mask, r2 = 16 (255 kept)", zones, min(int(nzones), 255))):
        if count == 0:
            continue
        dev.to_device(d_lab, labels)
        planes = max(int(count).bit_length(), 1)
        for r in (1, 2):
            changed = C.c_uint64(0)
            dev.check(lib.svr_region_label_smooth(p(d_lab), dims, count, u32(r, r, r), 1, p(d_lab_out), C.byref(changed)))
            t_mode = timed(lambda: dev.check(lib.svr_region_label_smooth(p(d_lab), dims, count, u32(r, r, r), 1, p(d_lab_out), None)), smooth_ms)
            f_planes = (4 * vox.size + 4 * planes * words) / HBM * 1e3
            yard = f_planes + (count + 1) * majority[("bone", r)]
            print(f"mode, {name}, r = {r}: {fmt(t_mode)} = {t_mode[0] / yard:5.2f} x (planes floor {f_planes:.4f} ms + {count + 1} x majority {majority[('bone', r)]:.4f} ms); "
                  f"{single_label_tiles(labels, r) * 100:.1f} % of the tiles hold one label; {changed.value} voxels change", flush=True)
    # ---- what the smoothing does to the surface: the mesh before and after MAJORITY of radius 1, of the bone mask (d_mask holds it) and of
    # a ragged one: the bone window of the voxels with noise of +- 4000 added, its largest 26-connected part
    def meshes(name):
        dev.check(lib.svr_region_smooth(p(d_mask), dims, abi.SMOOTH_MAJORITY, u32(1, 1, 1), 1, p(d_out), None))
        for what, ptr in ((name, d_mask), ("after majority r = 1", d_out)):
            v, t, _ = dev.mesh_region(ptr, shape=shape)
            vol6, area = dev.mesh_measure(v, t)
            print(f"mesh of {what}: {len(v)} vertices, {len(t)} triangles, volume {vol6 / (6 * 256 ** 3):.1f} voxels, area {area:.1f} voxel faces", flush=True)
    meshes("the bone mask")
    noisy = np.clip(vox.astype(np.int32) + np.random.default_rng(1).integers(-4000, 4001, shape, dtype=np.int32), 0, 65535).astype(np.uint16)
    dev.to_device(d_u16, noisy)
    dev.check(lib.svr_region_threshold(p(d_u16), n, n, n, 1, 39321, 65535, None, None, p(d_out)))
    dev.check(lib.svr_region_label(p(d_out), n, n, n, 26, p(d_lab), C.byref(k)))
    largest, kept = dev.region_select_by_size(d_lab, int(k.value), largest_k=1, shape=shape, out_ptr=d_mask)
    print(f"noisy bone window: {k.value} parts, the largest has {int(largest.sum())} voxels", flush=True)
    meshes("the largest part of the noisy bone window")
    for ptr in (d_vox, d_u16, d_full, d_mask, d_out, d_lab, d_lab_out):
        dev.free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a size may take")
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
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
