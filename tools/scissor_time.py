#!/usr/bin/env python3
"""Time the scissor calls (svr_stencil_polygon, svr_region_scissor_camera / _slice) on the phantom head.  Per row the HIP-event time of the
call's device work (svr_region_scissor_last_ms), median of 5 calls after a warm-up (min .. max), next to yardsticks from the same job:
  svr_stencil_polygon        at 1024 x 1024 for 4, 64 and 4096 vertices (a star-shaped ring around the image centre);
  the prism                  through the c3 camera (1024 x 1024, a ring stencil of 64 vertices) and through the axial slice at 0.5 within
                             a slab of 32 voxels: SELECT, ERASE_INSIDE of the brain and of the bone window's mask, FILL_INSIDE of the
                             brain window's mask;
  against                    svr_region_threshold of the same volume (one lane per voxel, 2 B read, a bit written; svr_region_label_last_ms),
                             svr_region_combine AND of the two masks (svr_region_mask_last_ms), and the byte floor of 1 bit in + 1 bit
                             out per voxel at 8 TB/s.
The size runs in a child process under its own time limit, so one that goes wrong ends alone.
usage: tools/scissor_time.py [--n 512] [--limit SECONDS]"""
import argparse
import ctypes as C
import math
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM = 8e12                                               # bytes / s


def ring(cx, cy, n, r0, r1, lobes=7):
    import numpy as np
    a = 2.0 * math.pi * np.arange(n) / n
    r = r0 + r1 * np.sin(lobes * a)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=-1)


def child(n: int):
    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    sc = scenes.make_scene("c3", n=n)                   # the c3 phantom and its camera (n = 512 is c3 itself)
    vox = sc.vox
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    voxels = vox.size
    words = host.region_mask_words(shape)
    W, H = sc.width, sc.height
    cam = sc.resolved_camera()
    vol = host.create_device_volume(0, sc.dim, sc.spacing, 1.0)
    sl = host.slice_params_axis(lib, vol, 2, 0.5, W, H)
    d_vox = dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    d_brain, d_bone, d_out = (dev.malloc(4 * words) for _ in range(3))
    d_st = dev.malloc(4 * host.region_mask_words((1, H, W)))
    ms = C.c_float()
    p = lambda ptr: C.c_void_p(ptr)                      # noqa: E731

    def timed(call, last_ms, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            dev.check(last_ms(C.byref(ms)))
            t.append(ms.value)
        return statistics.median(t), min(t), max(t)

    def fmt(t):
        return f"{t[0]:8.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"

    dev.check(lib.svr_region_threshold(p(d_vox), n, n, n, 1, 23593, 28835, None, None, p(d_brain)))
    dev.check(lib.svr_region_threshold(p(d_vox), n, n, n, 1, 39321, 65535, None, None, p(d_bone)))
    dev.synchronize()
    y_thr = timed(lambda: dev.check(lib.svr_region_threshold(p(d_vox), n, n, n, 1, 23593, 28835, None, None, p(d_out))), lib.svr_region_label_last_ms)
    y_and = timed(lambda: dev.check(lib.svr_region_combine(p(d_brain), p(d_bone), n, n, n, abi.MASK_AND, p(d_out))), lib.svr_region_mask_last_ms)
    floor = 2 * voxels / 8 / HBM * 1e3
    print(f"{n}^3 yardsticks: threshold {fmt(y_thr)}; combine and {fmt(y_and)}; byte floor (1 bit in + 1 bit out per voxel) {floor:.4f} ms", flush=True)
    for name, d_m in (("brain", d_brain), ("bone", d_bone)):
        m = dev.to_host(d_m, (words,), np.uint32)
        print(f"{n}^3 {name} mask: {int(np.unpackbits(m.view(np.uint8)).sum())} voxels = {100.0 * np.unpackbits(m.view(np.uint8)).sum() / voxels:.2f} %, "
              f"{int(np.count_nonzero(m))} of {words} words non-zero", flush=True)

    # the stencil
    for nv in (4, 64, 4096):
        contour = ring(0.5 * W, 0.5 * H, nv, 0.3 * W, 0.06 * W) if nv > 4 else host.stencil_rect(W // 4, H // 4, 3 * W // 4, 3 * H // 4, lib)
        q8 = np.ascontiguousarray(np.rint(contour * 256.0).astype(np.int32))
        counts = (C.c_uint32 * 1)(nv)
        t = timed(lambda: dev.check(lib.svr_stencil_polygon(q8.ctypes.data_as(C.POINTER(C.c_int32)), counts, 1, W, H, p(d_st))), lib.svr_region_scissor_last_ms)
        print(f"{W} x {H} stencil, {nv:4d} vertices: {fmt(t)}", flush=True)
    dev.stencil_polygon([ring(0.5 * W, 0.5 * H, 64, 0.3 * W, 0.06 * W)], W, H, out_ptr=d_st)

    # the prism
    slab = 32.0 * sc.spacing[2]
    for view, call, tail, depth in (("camera c3", lib.svr_region_scissor_camera, (C.byref(cam),), (-math.inf, math.inf)),
                                    ("axial slice, slab of 32", lib.svr_region_scissor_slice, (C.byref(sl), W, H), (-0.5 * slab, 0.5 * slab))):
        times = {}
        for what, op, d_in in (("select", abi.SCISSOR_SELECT, None), ("erase inside, brain", abi.SCISSOR_ERASE_INSIDE, d_brain),
                               ("erase inside, bone", abi.SCISSOR_ERASE_INSIDE, d_bone), ("fill inside, brain", abi.SCISSOR_FILL_INSIDE, d_brain)):
            sp = host.scissor_params(op, depth)
            t = timed(lambda: dev.check(call(None if d_in is None else p(d_in), n, n, n, C.byref(vol), *tail, p(d_st), C.byref(sp), p(d_out))),
                      lib.svr_region_scissor_last_ms)
            times[what] = t[0]
            got = dev.to_host(d_out, (words,), np.uint32)
            print(f"{n}^3 {view}, {what:20s}: {fmt(t)} = {t[0] / y_thr[0]:6.2f} x threshold, {t[0] / y_and[0]:6.2f} x combine, {t[0] / floor:6.1f} x floor; "
                  f"{int(np.unpackbits(got.view(np.uint8)).sum())} voxels out", flush=True)
        print(f"{n}^3 {view}: erase inside of the bone mask / select = {times['erase inside, bone'] / times['select']:.2f} (the word-driven skip)", flush=True)
    for ptr in (d_vox, d_brain, d_bone, d_out, d_st):
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
