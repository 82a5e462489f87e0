#!/usr/bin/env python3
"""Time the histogram calls (svr_volume_histogram, svr_region_label_histogram) on the phantom head and write profiles/histogram_times.txt:
the whole volume at shift 0 (65536 bins: two passes of LDS counters) and shift 8 (256 bins), inside the brain and bone masks of
tools/region_time.py, the per-label table of the parts of the bone window (shift 8), and an all-equal volume of the same size, the worst
contention.  Per row the HIP-event time of the call's device work (svr_volume_histogram_last_ms: the memset of the counters and the
kernel), median of 5 calls after a warm-up, and the ratio to the byte floor at 8 TB/s (the HBM rate of DESIGN.md section 6): 2 B per
voxel, plus 1/8 B with a mask, plus 4 B with labels.  From the same job, as yardsticks: svr_region_stats_of on the same masks, which
reads the same bytes (wall time of the call, which ends in a read-back), and the load-time pass svr_volume_preprocess of the same volume
as int16 (svr_volume_preprocess_last_ms: cast / range / gradient pass plus the rescale-and-histogram pass, with its own byte count).
One job, one process, under its own time limit.
usage: tools/histogram_time.py [--n 512] [--out profiles/histogram_times.txt] [--limit SECONDS]"""
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


def child(n: int, out_path: str):
    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    vox, _ = scenes._volume("head", n)                  # the c3 (512) phantom, without its gradient pass
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    voxels = vox.size
    words = host.region_mask_words(shape)
    dims = (C.c_int32 * 3)(shape[2], shape[1], shape[0])
    d_vox, d_flat = dev.malloc(vox.nbytes), dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    d_mask, d_labels = dev.malloc(4 * words), dev.malloc(4 * voxels)
    d_out = dev.malloc(4 * abi.HISTOGRAM_MAX_CELLS)
    ms = C.c_float()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(call, reps=5):
        call()
        t = []
        for _ in range(reps):
            call()
            dev.check(lib.svr_volume_histogram_last_ms(C.byref(ms)))
            t.append(ms.value)
        return statistics.median(t), min(t), max(t)

    def wall(call, reps=5):
        call()
        t = []
        for _ in range(reps):
            dev.synchronize()
            t0 = time.perf_counter()
            call()
            dev.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t)

    def hist(src, mask, shift):
        p = dev.histogram_params(shift=shift)
        return lambda: dev.check(lib.svr_volume_histogram(C.c_void_p(src), dims, 1, C.c_void_p(mask) if mask else None, C.byref(p), C.c_void_p(d_out)))

    say(f"# tools/histogram_time.py --n {n}: {lib.svr_device_info().decode()}; median of 5 calls (min .. max), floor at {HBM / 1e12:.0f} TB/s")
    floor = 2 * voxels / HBM * 1e3
    whole = {}
    for shift in (0, 8):
        t = timed(hist(d_vox, None, shift))
        whole[shift] = t[0]
        bins = 65536 >> shift
        check = dev.to_host(d_out, (bins,), np.uint32)
        assert int(check.sum(dtype=np.uint64)) == voxels
        say(f"{n}^3 head whole volume shift {shift} ({bins} bins): {t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; {t[0] / floor:5.1f} x floor), "
            f"{int(check[0]) * 100.0 / voxels:.1f} % in bin 0, {int((check > 0).sum())} bins occupied")

    for name, lo, hi in (("brain", 23593, 28835), ("bone", 39321, 65535)):
        dev.check(lib.svr_region_threshold(C.c_void_p(d_vox), shape[2], shape[1], shape[0], 1, lo, hi, None, None, C.c_void_p(d_mask)))
        st = dev.region_stats_of(d_vox, d_mask, shape=shape)
        t_stats = wall(lambda: dev.region_stats_of(d_vox, d_mask, shape=shape))
        mfloor = (2 * voxels + 4 * words) / HBM * 1e3
        for shift in (0, 8):
            t = timed(hist(d_vox, d_mask, shift))
            check = dev.to_host(d_out, (65536 >> shift,), np.uint32)
            assert int(check.sum(dtype=np.uint64)) == int(st.voxels)
            say(f"{n}^3 head inside the {name} mask ({int(st.voxels)} voxels) shift {shift}: {t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; "
                f"{t[0] / mfloor:5.1f} x floor; {t[0] / t_stats:5.2f} x svr_region_stats_of)")
        say(f"{n}^3 head svr_region_stats_of on the {name} mask: {t_stats:7.3f} ms wall ({t_stats / mfloor:5.1f} x floor)")
        if name == "bone":
            k = C.c_uint32()
            dev.check(lib.svr_region_label(C.c_void_p(d_mask), shape[2], shape[1], shape[0], 6, C.c_void_p(d_labels), C.byref(k)))
            p = dev.histogram_params(shift=8)
            lfloor = 6 * voxels / HBM * 1e3
            t = timed(lambda: dev.check(lib.svr_region_label_histogram(C.c_void_p(d_labels), C.c_void_p(d_vox), dims, 1, k.value, C.byref(p),
                                                                      C.c_void_p(d_out))))
            table = dev.to_host(d_out, (k.value + 1, 256), np.uint32)
            assert int(table[1:].sum(dtype=np.uint64)) == int(st.voxels)
            say(f"{n}^3 head per-label table of the {k.value} parts of the bone window, shift 8 ({(k.value + 1) * 256} cells): {t[0]:7.3f} ms "
                f"({t[1]:.3f} .. {t[2]:.3f}; {t[0] / lfloor:5.1f} x floor)")

    dev.check(lib.svr_memset_device(C.c_void_p(d_flat), 0x11, vox.nbytes))      # every voxel 0x1111
    for shift in (0, 8):
        t = timed(hist(d_flat, None, shift))
        check = dev.to_host(d_out, (65536 >> shift,), np.uint32)
        assert int(check[0x1111 >> shift]) == voxels
        say(f"{n}^3 all-equal volume shift {shift}: {t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f}; {t[0] / floor:5.1f} x floor; "
            f"{t[0] / whole[shift]:5.2f} x the head)")

    # the load-time pass on the same volume as int16 elements on the device
    i16 = (vox.astype(np.int32) - 32768).astype(np.int16)
    d_i16 = dev.malloc(i16.nbytes)
    dev.to_device(d_i16, i16)
    info = abi.VolumeInfo()
    sp = (C.c_double * 3)(1.0, 1.0, 1.0)
    hist_host = np.zeros(65536, np.uint32)
    t, nbytes = [], C.c_uint64()
    for _ in range(6):
        dev.check(lib.svr_volume_preprocess(C.c_void_p(d_i16), abi.ELEM_I16, shape[2], shape[1], shape[0], sp, 1, C.c_void_p(d_flat),
                                            hist_host.ctypes.data_as(C.c_void_p), 65536, C.byref(info)))
        dev.check(lib.svr_volume_preprocess_last_ms(C.byref(ms), C.byref(nbytes)))
        t.append(ms.value)
    pre = statistics.median(t[1:])
    say(f"{n}^3 head svr_volume_preprocess (int16; both passes, {nbytes.value / voxels:.0f} B / voxel, {int(info.hist_bins)} bins): {pre:7.3f} ms "
        f"({pre / (nbytes.value / HBM * 1e3):5.1f} x its floor); the whole-volume histogram at shift 0 is {whole[0] / pre:.5f} x that")
    for ptr in (d_vox, d_flat, d_mask, d_labels, d_out, d_i16):
        dev.free(ptr)
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "histogram_times.txt"))
    ap.add_argument("--limit", type=float, default=300.0, help="seconds the job may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.n, a.out)
        return 0
    try:
        rc = subprocess.run([sys.executable, __file__, "--child", "--n", str(a.n), "--out", a.out], timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        print(f"{a.n}^3: not finished after {a.limit:.0f} s", flush=True)
        return 1
    if rc != 0:
        print(f"{a.n}^3: exit status {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
