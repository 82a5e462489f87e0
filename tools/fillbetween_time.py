#!/usr/bin/env python3
"""Time fill between slices (svr_region_slice_counts, svr_region_slice_distance, svr_region_fill_between) on the phantom head.  The brain
and bone windows' masks keep every 4th or every 16th slice of the fill axis (z, then x) and are filled again.  Per row the HIP-event
times, median of 5 calls after a warm-up (min .. max):
  counts      svr_region_slice_counts (svr_region_fill_between_last_ms), against reading the mask once at 8 TB/s;
  maps        svr_region_slice_distance of the keys, against its 4 B written per voxel of the key slices;
  fill        the fill pass inside svr_region_fill_between (svr_region_fill_between_pass_ms), against its byte floor: 8 B of maps read
              and 1 bit written per filled voxel, plus the mask read and written once;
  whole       svr_region_fill_between (svr_region_fill_between_last_ms): two counts, the maps, the table and the fill, without the
              allocations and the wait between the first count and the rest;
  against     svr_region_distance of the full mask and one svr_region_combine, in the same job; the Dice of the sparse and of the filled
              mask against the full one.
The size runs in a child process under its own time limit, so one that goes wrong ends alone.
usage: tools/fillbetween_time.py [--n 512] [--limit SECONDS]"""
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
    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    vox = scenes.make_scene("c3", n=n).vox               # the c3 phantom (n = 512 is c3 itself)
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    words = host.region_mask_words(shape)
    plane = n * n
    ms = C.c_float()
    p = lambda ptr: C.c_void_p(ptr)                      # noqa: E731

    def timed(call, read, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            t.append(read())
        return statistics.median(t), min(t), max(t)

    def last(fn):
        def read():
            dev.check(fn(C.byref(ms)))
            return ms.value
        return read

    def fmt(t):
        return f"{t[0]:8.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"

    def dice(a, b):
        both, a_only, b_only, _ = dev.region_overlap(a, b, shape=shape)
        return 2.0 * both / max(2 * both + a_only + b_only, 1)

    d_vox = dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    d_full, d_sparse, d_out = (dev.malloc(4 * words) for _ in range(3))
    d_map = dev.malloc(4 * vox.size)
    counts = (C.c_uint64 * n)()
    for window, lo, hi in (("brain", 23593, 28835), ("bone", 39321, 65535)):
        dev.check(lib.svr_region_threshold(p(d_vox), n, n, n, 1, lo, hi, None, None, p(d_full)))
        dev.synchronize()
        full = host.region_mask_unpack(dev.to_host(d_full, (words,), np.uint32), shape)
        y_dist = timed(lambda: dev.check(lib.svr_region_distance(p(d_full), n, n, n, None, abi.DIST_TO_SET, p(d_map))), last(lib.svr_region_distance_last_ms))
        y_or = timed(lambda: dev.check(lib.svr_region_combine(p(d_full), p(d_full), n, n, n, abi.MASK_OR, p(d_out))), last(lib.svr_region_mask_last_ms))
        print(f"{n}^3 {window}: {int(full.sum())} voxels; svr_region_distance TO_SET {fmt(y_dist)}; svr_region_combine {fmt(y_or)}", flush=True)
        for axis in (2, 0):
            for every in (4, 16):
                sparse = full.copy()
                np.moveaxis(sparse, 2 - axis, 0)[np.arange(n) % every != 0] = False
                dev.to_device(d_sparse, host.region_mask_pack(sparse))
                params = host.fill_between_params(axis)
                info = abi.FillBetweenInfo()
                fill = lambda: dev.check(lib.svr_region_fill_between(p(d_sparse), n, n, n, C.byref(params), p(d_out), C.byref(info)))   # noqa: E731
                t_whole = timed(fill, last(lib.svr_region_fill_between_last_ms))
                passes = [timed(fill, lambda i=i: dev.region_fill_between_pass_ms()[i]) for i in range(3)]
                t_counts = timed(lambda: dev.check(lib.svr_region_slice_counts(p(d_sparse), n, n, n, axis, counts)), last(lib.svr_region_fill_between_last_ms))
                keys = np.ascontiguousarray(np.nonzero(np.array(list(counts)))[0], dtype=np.int32)
                t_maps = timed(lambda: dev.check(lib.svr_region_slice_distance(p(d_sparse), n, n, n, axis, None, keys.ctypes.data_as(C.POINTER(C.c_int32)), len(keys),
                                                                               p(d_map))), last(lib.svr_region_fill_between_last_ms))
                filled_voxels = info.filled_slices * plane
                f_counts, f_maps = 4 * words / HBM * 1e3, 4 * len(keys) * plane / HBM * 1e3
                f_fill = (8 * filled_voxels + filled_voxels / 8 + 8 * words) / HBM * 1e3
                print(f"{n}^3 {window}, axis {'xyz'[axis]}, every {every:2d}th slice: {info.keys} keys, {info.gaps} gaps, {info.filled_slices} slices filled, "
                      f"{info.voxels_in} -> {info.voxels_out} voxels, Dice {dice(d_sparse, d_full):.4f} -> {dice(d_out, d_full):.4f}, "
                      f"workspace {info.workspace_bytes / 2 ** 20:.0f} MiB, {info.launches} launch", flush=True)
                print(f"    counts {fmt(t_counts)} = {t_counts[0] / f_counts:6.1f} x floor, {t_counts[0] / y_or[0]:5.2f} x combine", flush=True)
                print(f"    maps   {fmt(t_maps)} = {t_maps[0] / f_maps:6.1f} x floor; per key slice {t_maps[0] / len(keys):.4f} ms; "
                      f"svr_region_distance per slice {y_dist[0] / n:.4f} ms", flush=True)
                print(f"    fill   {fmt(passes[2])} = {passes[2][0] / f_fill:6.1f} x floor, {passes[2][0] / y_or[0]:5.2f} x combine  "
                      f"(inside the call: counts {passes[0][0]:.4f} ms, maps {passes[1][0]:.4f} ms)", flush=True)
                print(f"    whole  {fmt(t_whole)} = {t_whole[0] / y_dist[0]:5.2f} x svr_region_distance of the full mask", flush=True)
    for ptr in (d_vox, d_full, d_sparse, d_out, d_map):
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
