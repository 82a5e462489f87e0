#!/usr/bin/env python3
"""Time grow-from-seeds (svr_region_growcut) on the phantom head of scene c3: strokes of three classes -- brain, bone, air, each a ball of
radius 3 voxels painted with svr_region_ball and svr_region_label_paint around a voxel of the class -- grown over the whole volume and over
the brain window's mask.  Per row the HIP-event time of the call's device work (svr_region_growcut_last_ms: the launches, without the
hipMalloc / hipFree of the workspace), median of 3 calls after a warm-up, the sweeps launched, the unreached and saturated counts, the
class sizes and a checksum of the zones:
  svr_region_growcut with the default weights of connectivity 26 and contrast_gain 1 at contrast_shift 0 and 4;
  the same call with contrast_gain 0, which computes what svr_region_geodesic computes: the cost of loading and reading the value tile;
  svr_region_geodesic (svr_region_geodesic_last_ms) on the same markers, domain and weights, in the same job.  The whole volume is a full
    mask there.  The ratios growcut / geodesic and growcut(gain 0) / geodesic are printed, and whether the gain 0 zones equal the
    geodesic ones.
A run that needs more than the default sweep cap is repeated with max_sweeps 65536 and the cap it needed is in its row.
Every size runs in a child process under its own time limit, so one that goes wrong ends alone.  The lines go to stdout and to --out.
usage: tools/growcut_time.py [--n 512] [--limit SECONDS] [--out profiles/growcut_times.txt]"""
import argparse
import ctypes as C
import statistics
import subprocess
import sys
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REPS = 3
STROKE_R2 = 9                                            # a ball of radius 3 voxels
WINDOWS = {"brain": (23593, 28835), "bone": (39321, 65535)}          # the raw windows of tools/distance_time.py


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
    dims = (C.c_int32 * 3)(n, n, n)
    d_vox = dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    d_brain, d_full, d_point, d_stroke = (dev.malloc(4 * words) for _ in range(4))
    d_markers, d_cost, d_zones, d_geo = (dev.malloc(4 * voxels) for _ in range(4))
    ms = C.c_float()

    def last(fn):
        dev.check(fn(C.byref(ms)))
        return ms.value

    def crc(ptr):
        return zlib.crc32(dev.to_host(ptr, (voxels,), np.uint32).tobytes())

    # ---- the strokes
    dev.check(lib.svr_memset_device(C.c_void_p(d_markers), 0, 4 * voxels))
    dev.check(lib.svr_region_threshold(C.c_void_p(d_vox), n, n, n, 1, 0, 65535, None, None, C.c_void_p(d_full)))
    seeds = {}
    for cls, name in enumerate(("brain", "bone", "air"), start=1):
        if name == "air":
            seed = (2, 2, 2)
        else:
            lo, hi = WINDOWS[name]
            mask = dev.region_threshold(d_vox, lo, hi, shape=shape, out_ptr=d_brain if name == "brain" else None)
            at = np.argwhere(mask)
            seed = tuple(int(t) for t in at[np.argmin(((at - at.mean(axis=0)) ** 2).sum(axis=1))][::-1])     # (x, y, z): the voxel of the window nearest its centroid
        seeds[name] = seed
        point = np.zeros(words, dtype=np.uint32)
        point[(seed[2] * n + seed[1]) * ((n + 31) // 32) + seed[0] // 32] = 1 << (seed[0] % 32)
        dev.to_device(d_point, point)
        dev.check(lib.svr_region_ball(C.c_void_p(d_point), n, n, n, abi.MORPH_DILATE, None, STROKE_R2, C.c_void_p(d_stroke)))
        dev.check(lib.svr_region_label_paint(C.c_void_p(d_markers), dims, C.c_void_p(d_stroke), cls, 1))
    dev.synchronize()
    markers = dev.to_host(d_markers, shape, np.uint32)
    print(f"{n}^3: strokes of r2 {STROKE_R2} at " + ", ".join(f"{k} {v} (raw {int(vox[v[2], v[1], v[0]])})" for k, v in seeds.items())
          + f": {np.bincount(markers.reshape(-1))[1:].tolist()} marker voxels; default sweep cap {lib.svr_region_geodesic_default_max_sweeps(n, n, n)}", flush=True)

    weights = (1,) * 7
    cw = (C.c_uint32 * 7)(*weights)
    for dname, d_dom, d_geo_dom in (("whole volume", None, d_full), ("brain window", d_brain, d_brain)):
        sweeps = C.c_uint32()

        def geodesic():
            dev.check(lib.svr_region_geodesic(C.c_void_p(d_markers), C.c_void_p(d_geo_dom), n, n, n, cw, 0, None, C.c_void_p(d_geo), C.byref(sweeps)))
        geodesic()
        t = []
        for _ in range(REPS):
            geodesic()
            t.append(last(lib.svr_region_geodesic_last_ms))
        geo_ms = statistics.median(t)
        geo_zones = dev.to_host(d_geo, shape, np.uint32)
        print(f"{n}^3 {dname}: geodesic, weights 1 x 7: {geo_ms:9.3f} ms ({min(t):.3f} .. {max(t):.3f}), {int(sweeps.value)} sweeps, classes "
              f"{np.bincount(geo_zones.reshape(-1), minlength=4)[1:].tolist()}, crc {crc(d_geo):08x}", flush=True)
        for gain, shift in ((0, 0), (1, 4), (1, 0)):
            p = dev.growcut_params(weights, 26, gain, shift, 0)
            info = abi.GrowcutInfo()

            def grow():
                return lib.svr_region_growcut(C.c_void_p(d_vox), dims, 1, C.c_void_p(d_markers), None if d_dom is None else C.c_void_p(d_dom), C.byref(p),
                                              C.c_void_p(d_cost), C.c_void_p(d_zones), C.byref(info))
            rc = grow()
            cap = "default cap"
            if rc == abi.REGION_ERR_SWEEPS:                               # the default cap was not enough: say so and go on with the largest
                lib.svr_clear_error()
                p.max_sweeps = 65536
                rc = grow()
                cap = "max_sweeps 65536 (the default cap was NOT enough)"
            if rc not in (0, abi.REGION_ERR_RANGE):
                dev.check(rc)
            lib.svr_clear_error()
            t = []
            for _ in range(REPS):
                grow()
                lib.svr_clear_error()
                t.append(last(lib.svr_region_growcut_last_ms))
            g_ms = statistics.median(t)
            zones = dev.to_host(d_zones, shape, np.uint32)
            cost = dev.to_host(d_cost, shape, np.uint32)
            reached = cost != abi.GEO_NONE
            note = f"; zones equal the geodesic call's: {bool(np.array_equal(zones, geo_zones))}" if gain == 0 else ""
            print(f"{n}^3 {dname}: growcut gain {gain} shift {shift}: {g_ms:9.3f} ms ({min(t):.3f} .. {max(t):.3f}) = {g_ms / geo_ms:.2f} x geodesic, {info.sweeps} sweeps "
                  f"({cap}), unreached {info.unreached}, saturated {info.saturated}{' (SVR_REGION_ERR_RANGE)' if rc else ''}, max cost "
                  f"{int(cost[reached].max()) if reached.any() else 0}, classes {np.bincount(zones.reshape(-1), minlength=4)[1:].tolist()}, crc {crc(d_zones):08x}{note}",
                  flush=True)
    for ptr in (d_vox, d_brain, d_full, d_point, d_stroke, d_markers, d_cost, d_zones, d_geo):
        dev.free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--limit", type=float, default=400.0, help="seconds a size may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "growcut_times.txt"))
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
