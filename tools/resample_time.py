#!/usr/bin/env python3
"""Time the crop / resample calls (svr_volume_resample, svr_region_resample, svr_region_label_resample, svr_region_paste,
svr_region_mask_expand) on the phantom head of c3 (512^3).  Per row the HIP-event time of the call's device work
(svr_volume_resample_last_ms: the launches, without the hipMalloc / hipFree of the intermediate volumes), median of 5 calls after a
warm-up, the BYTE FLOOR of the call -- every pass reads its input once and writes its output once, at 8 TB/s (the HBM rate of DESIGN.md
section 6); a gather reads only the source voxels it needs -- and a checksum of the result.  The yardstick, from the same job, is
svr_volume_smooth at radii (1, 1, 1): three passes of existing code with the traffic of a pass that keeps the size.
Cases: the crop to the bone region's box (volume, mask, labels); AREA by 2 on all axes; isotropic resampling from a pretended (1, 1, 2)
spacing (AUTO: only z resamples, LINEAR); LINEAR x 2 of a 256^3 crop; the paste of the cropped mask; the expansion of the mask.
The measurement runs in a child process under a time limit, so one that goes wrong ends alone.
usage: tools/resample_time.py [--n 512] [--limit SECONDS]"""
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


def is_copy(m):
    return m[1] == 65536 and m[0] % 65536 == 0


def volume_floor_bytes(shape, grid, nearest):
    """The bytes svr_volume_resample has to move: per pass 2 B per voxel read and written; NEAREST and a crop are one gather that reads at
    most one source voxel per output voxel."""
    src = [shape[2], shape[1], shape[0]]
    dst = [m[2] for m in grid]
    out = dst[0] * dst[1] * dst[2]
    passes = [a for a in range(3) if not is_copy(grid[a])]
    if nearest or not passes:
        return 2 * (min(out, src[0] * src[1] * src[2]) + out), 1
    d = [dst[a] if is_copy(grid[a]) else src[a] for a in range(3)]
    total = 0
    for a in passes:
        read = d[0] * d[1] * d[2]
        if a == passes[0]:                               # the first pass also crops the copy axes: it reads the cells' source span only
            span = min(src[a], (grid[a][2] * grid[a][1] >> 16) + 2)
            read = read // d[a] * span
        d[a] = dst[a]
        total += 2 * (read + d[0] * d[1] * d[2])
    return total, len(passes)


def child(n: int):
    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    vox, _ = scenes._volume("head", n)                  # the c3 (512) phantom, without its gradient pass
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    voxels = vox.size
    dims = (C.c_int32 * 3)(n, n, n)
    d_vox, d_tmp = dev.malloc(vox.nbytes), dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    ms = C.c_float()

    def timed(call, last_ms, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            dev.check(last_ms(C.byref(ms)))
            t.append(ms.value)
        return statistics.median(t), min(t), max(t)

    def report(name, t, nbytes, passes, crc):
        floor = nbytes / HBM * 1e3
        print(f"{n}^3 {name:44s} {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}), {passes} pass(es), floor {floor:7.4f} ms, {t[0] / floor:6.1f} x floor, "
              f"{nbytes / (t[0] * 1e-3) / 1e9:7.0f} GB/s, crc {crc:08x}", flush=True)

    # the yardstick
    r = (C.c_uint32 * 3)(1, 1, 1)
    t = timed(lambda: dev.check(lib.svr_volume_smooth(C.c_void_p(d_vox), n, n, n, 1, r, C.c_void_p(d_tmp))), lib.svr_volume_filter_last_ms)
    report("svr_volume_smooth radii (1, 1, 1) [yardstick]", t, 3 * 4 * voxels, 3, zlib.crc32(dev.to_host(d_tmp, (voxels,), np.uint16).tobytes()))
    per_pass = t[0] / 3
    print(f"{n}^3 the yardstick's pass: {per_pass:.3f} ms = {per_pass / (4 * voxels / HBM * 1e3):.1f} x its floor", flush=True)
    dev.free(d_tmp)

    def volume_case(name, src_ptr, src_shape, grid, mode):
        g = host.resample_grid(grid)
        out = dev.malloc(2 * int(np.prod(g.shape)))
        sd = (C.c_int32 * 3)(*src_shape[::-1])
        t = timed(lambda: dev.check(lib.svr_volume_resample(C.c_void_p(src_ptr), sd, 1, C.byref(g), mode, C.c_void_p(out))), lib.svr_volume_resample_last_ms)
        nbytes, passes = volume_floor_bytes(src_shape, g.as_tuples(), mode == abi.RESAMPLE_NEAREST)
        report(f"{name} -> {g.shape[2]} x {g.shape[1]} x {g.shape[0]}", t, nbytes, passes, zlib.crc32(dev.to_host(out, g.shape, np.uint16).tobytes()))
        return out, g

    # the bone region, its box, its labels
    words = host.region_mask_words(shape)
    d_mask, d_labels = dev.malloc(4 * words), dev.malloc(4 * voxels)
    dev.check(lib.svr_region_threshold(C.c_void_p(d_vox), n, n, n, 1, 39321, 65535, None, None, C.c_void_p(d_mask)))
    st = dev.region_stats_of(d_vox, d_mask, shape=shape)
    k = C.c_uint32(0)
    dev.check(lib.svr_region_label(C.c_void_p(d_mask), n, n, n, 6, C.c_void_p(d_labels), C.byref(k)))
    box = (tuple(st.bbox_min), tuple(st.bbox_max))
    print(f"{n}^3 bone window: {st.voxels} voxels in {k.value} parts, box {box[0]} .. {box[1]}", flush=True)

    d_crop, g_crop = volume_case("crop to the bone box", d_vox, shape, host.resample_grid_box(shape, box), abi.RESAMPLE_NEAREST)
    cshape, cvox = g_crop.shape, int(np.prod(g_crop.shape))
    cwords = host.region_mask_words(cshape)
    d_cmask, d_clabels = dev.malloc(4 * cwords), dev.malloc(4 * cvox)
    t = timed(lambda: dev.check(lib.svr_region_resample(C.c_void_p(d_mask), dims, C.byref(g_crop), C.c_void_p(d_cmask))), lib.svr_volume_resample_last_ms)
    report("crop of the mask (funnel)", t, 8 * cwords, 1, zlib.crc32(dev.to_host(d_cmask, (cwords,), np.uint32).tobytes()))
    t = timed(lambda: dev.check(lib.svr_region_label_resample(C.c_void_p(d_labels), dims, C.byref(g_crop), C.c_void_p(d_clabels))), lib.svr_volume_resample_last_ms)
    report("crop of the labels", t, 8 * cvox, 1, zlib.crc32(dev.to_host(d_clabels, (cvox,), np.uint32).tobytes()))
    dev.free(d_clabels)
    dev.free(d_labels)

    out, _ = volume_case("AREA by 2 on all axes", d_vox, shape, host.resample_grid_dims(shape, (n // 2,) * 3), abi.RESAMPLE_AREA)
    dev.free(out)
    g_half = host.resample_grid_dims(shape, (n // 2,) * 3)
    d_hmask = dev.malloc(4 * host.region_mask_words(g_half.shape))
    t = timed(lambda: dev.check(lib.svr_region_resample(C.c_void_p(d_mask), dims, C.byref(g_half), C.c_void_p(d_hmask))), lib.svr_volume_resample_last_ms)
    hw = host.region_mask_words(g_half.shape)
    report("mask by 2 on all axes (general form)", t, 4 * hw + 4 * words // 4, 1, zlib.crc32(dev.to_host(d_hmask, (hw,), np.uint32).tobytes()))
    dev.free(d_hmask)
    out, _ = volume_case("isotropic from spacing (1, 1, 2), AUTO", d_vox, shape, host.resample_grid_spacing(shape, (1.0, 1.0, 2.0), 1.0)[0], abi.RESAMPLE_AUTO)
    dev.free(out)
    q = n // 4
    d_sub, g_sub = volume_case("crop to the central half", d_vox, shape, host.resample_grid_box(shape, ((q,) * 3, (q + n // 2 - 1,) * 3)), abi.RESAMPLE_NEAREST)
    out, _ = volume_case("LINEAR x 2 of that crop", d_sub, g_sub.shape, host.resample_grid_dims(g_sub.shape, (n,) * 3), abi.RESAMPLE_LINEAR)
    dev.free(out)
    dev.free(d_sub)

    # the paste of the cropped mask back, and the expansion of the full mask
    off = (C.c_int32 * 3)(*box[0])
    cd = (C.c_int32 * 3)(*cshape[::-1])
    for name, op in (("REPLACE", abi.PASTE_REPLACE), ("OR", abi.MASK_OR), ("ANDNOT", abi.MASK_ANDNOT)):
        t = timed(lambda: dev.check(lib.svr_region_paste(C.c_void_p(d_cmask), cd, C.c_void_p(d_mask), dims, off, op)), lib.svr_volume_resample_last_ms)
        report(f"paste {name} of the cropped mask", t, 12 * cwords, 1, zlib.crc32(dev.to_host(d_mask, (words,), np.uint32).tobytes()))
    dev.check(lib.svr_region_paste(C.c_void_p(d_cmask), cd, C.c_void_p(d_mask), dims, off, abi.PASTE_REPLACE))      # the bone mask again
    d_u8 = dev.malloc(voxels)
    t = timed(lambda: dev.check(lib.svr_region_mask_expand(C.c_void_p(d_mask), dims, 1, C.c_void_p(d_u8))), lib.svr_volume_resample_last_ms)
    report("expand the mask to u8", t, 4 * words + voxels, 1, zlib.crc32(dev.to_host(d_u8, (voxels,), np.uint8).tobytes()))
    for ptr in (d_vox, d_mask, d_crop, d_cmask, d_u8):
        dev.free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds the measurement may take")
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    try:
        rc = subprocess.run([sys.executable, __file__, "--child", str(a.n)], timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        print(f"{a.n}^3: not finished after {a.limit:.0f} s; stopping here", flush=True)
        return 1
    if rc != 0:
        print(f"{a.n}^3: exit status {rc}; stopping here", flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
