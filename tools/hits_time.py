#!/usr/bin/env python3
"""Time svr_render_hits on a scene (default c3): per mode, with SVR_OPT_EMPTY_SKIP 1 and 0, next to the picture each mode belongs to in
the same process (render_raycasting for OPACITY, svr_render_projection ISO / MIP for ISO / MAX), and a 1-pixel and a 4096-pixel svr_pick.
Per figure: 3 warm-up calls, then the median and the fastest of 5 batches of 10 calls (one synchronisation per batch).
usage: tools/hits_time.py [scene] [iso] [alpha]"""
import ctypes as C
import statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
from sunvolumerender_amd import abi, host, scenes
name = sys.argv[1] if len(sys.argv) > 1 else "c3"
iso = float(sys.argv[2]) if len(sys.argv) > 2 else 0.15
alpha = float(sys.argv[3]) if len(sys.argv) > 3 else 0.5
sc = scenes.make_scene(name)
dev = host.Device(0)
c = host.Canvas(dev, sc.width, sc.height)
scenes.apply_to_canvas(sc, c, 0)
lib = dev.lib
buf = dev.malloc(sc.width * sc.height * 40)
scene_args = (C.byref(c.deviceVolume), C.byref(c.transferFunction), C.byref(c.camera), C.c_float(c.stepSize))


def timed(paint, warm=3, batches=5, n=10):
    for _ in range(warm):
        paint()
    dev.synchronize()
    ms = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(n):
            paint()
        dev.synchronize()
        ms.append((time.perf_counter() - t0) / n * 1e3)
    return statistics.median(ms), min(ms)


def hits(p):
    dev.check(lib.svr_render_hits(C.c_void_p(buf), *scene_args, C.byref(p)))


tag = f"{name} {sc.width}x{sc.height}"
c.SetRenderMode(host.Canvas.RENDER_MODE_RAYCASTING)
med, best = timed(c.paint)
print(f"{tag} raycast                  : median {med:.3f} ms/frame, fastest {best:.3f}")
for mode, mname in ((abi.PROJ_ISO, f"iso {iso:g}"), (abi.PROJ_MIP, "mip")):
    med, best = timed(lambda: c.paint_projection(mode, iso=iso))
    print(f"{tag} projection {mname:8s}      : median {med:.3f} ms/frame, fastest {best:.3f}")
for mode, mname in ((abi.HIT_OPACITY, f"opacity {alpha:g}"), (abi.HIT_ISO, f"iso {iso:g}"), (abi.HIT_MAX, "max")):
    p = abi.HitParams(mode, alpha, iso)
    for skip in (1, 0):
        dev.set_option(abi.OPT_EMPTY_SKIP, skip)
        dev.set_option(abi.OPT_COUNT, 0)
        med, best = timed(lambda: hits(p))
        dev.set_option(abi.OPT_COUNT, 1); dev.reset_counters(); hits(p); cnt = dev.counters()
        dev.set_option(abi.OPT_COUNT, 0)
        print(f"{tag} hits {mname:12s} skip {skip}: median {med:.3f} ms/frame, fastest {best:.3f}  "
              f"steps={cnt['raycast_steps']} taps_executed={cnt['vol_taps_executed']} of {cnt['vol_taps']}")
dev.set_option(abi.OPT_EMPTY_SKIP, 1)
rng = np.random.default_rng(1)
for n in (1, abi.PICK_MAX):
    xy = np.ascontiguousarray(np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n)], axis=1), dtype=np.uint32)
    if n == 1:
        xy[0] = (sc.width // 2, sc.height // 2)
    for mode, mname in ((abi.HIT_OPACITY, f"opacity {alpha:g}"), (abi.HIT_ISO, f"iso {iso:g}"), (abi.HIT_MAX, "max")):
        p = abi.HitParams(mode, alpha, iso)
        med, best = timed(lambda: dev.check(lib.svr_pick(C.c_void_p(buf), xy.ctypes.data_as(C.POINTER(C.c_uint32)), n, *scene_args, C.byref(p))))
        print(f"{tag} pick of {n:4d} {mname:12s}: median {med:.3f} ms/call, fastest {best:.3f}")
dev.free(buf)
c.close()
