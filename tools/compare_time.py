#!/usr/bin/env python3
"""Time the comparison calls (svr_region_surface, _overlap, _label_overlap, svr_region_distance_summary / _quantile, svr_region_compare)
on the phantom head: the brain and bone windows of tools/distance_time.py against the same windows of the median-filtered volume
(svr_volume_rank, element 18, one pass).  Per row the HIP-event time of the call's device work (svr_region_compare_last_ms), median of 5
calls after a warm-up (min .. max), next to a yardstick from the same job:
  svr_region_surface            against svr_region_morph ERODE, element 6, radius 1 (svr_region_mask_last_ms);
  svr_region_overlap            against svr_region_combine AND (svr_region_mask_last_ms);
  svr_region_distance_summary   over a surface mask, against svr_region_distance_max over the same mask (svr_region_distance_last_ms) and
                                against its byte floor at 8 TB/s: the mask words, and 128 B of the map for every non-zero word;
  svr_region_distance_quantile  over the same mask (a summary and one or two histogram passes);
  svr_region_label_overlap      of the parts of the window and of the filtered window (counts capped at 255), against
                                svr_region_label_histogram of the same labels at 256 bins (svr_volume_histogram_last_ms);
  svr_region_compare            whole, against two svr_region_distance calls (svr_region_distance_last_ms).
The size runs in a child process under its own time limit, so one that goes wrong ends alone.
usage: tools/compare_time.py [--n 512] [--limit SECONDS]"""
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

    vox, _ = scenes._volume("head", n)                  # the c3 (512) phantom, without its gradient pass
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    voxels = vox.size
    words = host.region_mask_words(shape)
    d_vox, d_med = dev.malloc(vox.nbytes), dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    dev.volume_median(d_vox, 18, 1, shape=shape, out_ptr=d_med)
    d_a, d_b, d_sa, d_sb, d_out = (dev.malloc(4 * words) for _ in range(5))
    d_map, d_la, d_lb = (dev.malloc(4 * voxels) for _ in range(3))
    d_table = dev.malloc(4 * 256 * 256)
    ms = C.c_float()
    dims = (C.c_int32 * 3)(n, n, n)

    def timed(call, last_ms, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            dev.check(last_ms(C.byref(ms)))
            t.append(ms.value)
        return statistics.median(t), min(t), max(t)

    def row(name, what, t, yard_name, y, extra=""):
        print(f"{n}^3 {name:5s} {what}: {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}) = {t[0] / y[0]:6.2f} x {yard_name} {y[0]:.3f} ms ({y[1]:.3f} .. {y[2]:.3f}){extra}",
              flush=True)

    p = lambda ptr: C.c_void_p(ptr)                      # noqa: E731
    for name, lo, hi in (("brain", 23593, 28835), ("bone", 39321, 65535)):
        dev.check(lib.svr_region_threshold(p(d_vox), n, n, n, 1, lo, hi, None, None, p(d_a)))
        dev.check(lib.svr_region_threshold(p(d_med), n, n, n, 1, lo, hi, None, None, p(d_b)))
        dev.synchronize()
        # the surface against one erosion step
        t = timed(lambda: dev.check(lib.svr_region_surface(p(d_a), n, n, n, 6, p(d_sa))), lib.svr_region_compare_last_ms)
        y = timed(lambda: dev.check(lib.svr_region_morph(p(d_a), n, n, n, abi.MORPH_ERODE, 6, 1, p(d_out))), lib.svr_region_mask_last_ms)
        row(name, "surface element  6", t, "morph erode 6 radius 1", y)
        t = timed(lambda: dev.check(lib.svr_region_surface(p(d_a), n, n, n, 26, p(d_sa))), lib.svr_region_compare_last_ms)
        y = timed(lambda: dev.check(lib.svr_region_morph(p(d_a), n, n, n, abi.MORPH_ERODE, 26, 1, p(d_out))), lib.svr_region_mask_last_ms)
        row(name, "surface element 26", t, "morph erode 26 radius 1", y)
        dev.check(lib.svr_region_surface(p(d_a), n, n, n, 6, p(d_sa)))
        dev.check(lib.svr_region_surface(p(d_b), n, n, n, 6, p(d_sb)))
        # the overlap counts against one set operation
        counts = (C.c_uint64 * 4)()
        t = timed(lambda: dev.check(lib.svr_region_overlap(p(d_a), p(d_b), n, n, n, None, counts)), lib.svr_region_compare_last_ms)
        y = timed(lambda: dev.check(lib.svr_region_combine(p(d_a), p(d_b), n, n, n, abi.MASK_AND, p(d_out))), lib.svr_region_mask_last_ms)
        row(name, "overlap", t, "combine and", y, f"; both {counts[0]} a only {counts[1]} b only {counts[2]} neither {counts[3]}")
        # the summary of the distances to S(B) over S(A) against distance_max over the same mask, and its byte floor
        dev.check(lib.svr_region_distance(p(d_sb), n, n, n, None, abi.DIST_TO_SET, p(d_map)))
        sa_words = dev.to_host(d_sa, (words,), np.uint32)
        nonzero, surface = int(np.count_nonzero(sa_words)), int(np.unpackbits(sa_words.view(np.uint8)).sum())
        floor = (4 * words + 128 * nonzero) / HBM * 1e3
        s = abi.DistanceSummary()
        tol = (C.c_uint32 * 3)(0, 1, 4)
        t = timed(lambda: dev.check(lib.svr_region_distance_summary(p(d_map), p(d_sa), n, n, n, tol, 3, C.byref(s))), lib.svr_region_compare_last_ms)
        m, first, status = C.c_uint32(), C.c_uint32(), C.c_int32()
        y = timed(lambda: dev.check(lib.svr_region_distance_max(p(d_map), p(d_sa), n, n, n, C.byref(m), C.byref(first), C.byref(status))),
                  lib.svr_region_distance_last_ms)
        assert (s.max, s.first_max) == (m.value, first.value)
        row(name, "summary over S(A)", t, "distance_max", y,
            f"; {t[0] / floor:5.1f} x floor {floor:.4f} ms ({surface} surface voxels = {100.0 * surface / voxels:.2f} % in {nonzero} of {words} words); max d2 {s.max} "
            f"at {s.first_max}, sum {s.sum}, root q8 {s.sum_root_q8}, within {list(s.within)[:3]}")
        q, qs = C.c_uint32(), C.c_int32()
        t = timed(lambda: dev.check(lib.svr_region_distance_quantile(p(d_map), p(d_sa), dims, 95, 100, C.byref(q), C.byref(qs))), lib.svr_region_compare_last_ms)
        row(name, "quantile 95 % over S(A)", t, "distance_max", y, f"; d2 {q.value}")
        ts = timed(lambda: dev.check(lib.svr_region_distance_summary(p(d_map), None, n, n, n, tol, 3, C.byref(s))), lib.svr_region_compare_last_ms)
        ym = timed(lambda: dev.check(lib.svr_region_distance_max(p(d_map), None, n, n, n, C.byref(m), C.byref(first), C.byref(status))),
                   lib.svr_region_distance_last_ms)
        row(name, "summary, no mask", ts, "distance_max, no mask", ym, f"; {ts[0] / (4 * voxels / HBM * 1e3):5.1f} x floor {4 * voxels / HBM * 1e3:.3f} ms")
        # the label table against the label histogram at 256 bins
        ka, kb = C.c_uint32(), C.c_uint32()
        dev.check(lib.svr_region_label(p(d_a), n, n, n, 6, p(d_la), C.byref(ka)))
        dev.check(lib.svr_region_label(p(d_b), n, n, n, 6, p(d_lb), C.byref(kb)))
        ca, cb = min(int(ka.value), 255) or 1, min(int(kb.value), 255) or 1
        t = timed(lambda: dev.check(lib.svr_region_label_overlap(p(d_la), ca, p(d_lb), cb, dims, p(d_table))), lib.svr_region_compare_last_ms)
        hp = dev.histogram_params(shift=8)
        y = timed(lambda: dev.check(lib.svr_region_label_histogram(p(d_la), p(d_vox), dims, 1, ca, C.byref(hp), p(d_table))),
                  lib.svr_volume_histogram_last_ms)
        row(name, f"label table {ca + 1} x {cb + 1} (of {ka.value} and {kb.value} parts)", t, f"label histogram {ca + 1} x 256", y,
            f"; {t[0] / (8 * voxels / HBM * 1e3):5.1f} x floor {8 * voxels / HBM * 1e3:.3f} ms")
        # the whole comparison against two distance transforms
        cp, out = host.compare_params(6, None, (95, 100), (0, 1, 4), lib), abi.RegionComparison()
        t = timed(lambda: dev.check(lib.svr_region_compare(p(d_a), p(d_b), n, n, n, C.byref(cp), C.byref(out))), lib.svr_region_compare_last_ms)
        y1 = timed(lambda: dev.check(lib.svr_region_distance(p(d_sb), n, n, n, None, abi.DIST_TO_SET, p(d_map))), lib.svr_region_distance_last_ms)
        y2 = timed(lambda: dev.check(lib.svr_region_distance(p(d_sa), n, n, n, None, abi.DIST_TO_SET, p(d_map))), lib.svr_region_distance_last_ms)
        y = tuple(a + b for a, b in zip(y1, y2))
        meas = host.compare_measure(out, 1.0, lib)
        row(name, "compare, whole", t, "two distance transforms", y,
            f"; dice {meas.dice:.4f} jaccard {meas.jaccard:.4f} hd {meas.hausdorff:.3f} hd95 {meas.hausdorff_q:.3f} assd {meas.assd:.4f} voxels, surfaces "
            f"{out.surface[0]} / {out.surface[1]}, surface dice {[round(v, 4) for v in list(meas.surface_dice)[:3]]}")
    for ptr in (d_vox, d_med, d_a, d_b, d_sa, d_sb, d_out, d_map, d_la, d_lb, d_table):
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
