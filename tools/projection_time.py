#!/usr/bin/env python3
"""Time svr_render_projection on a scene (default c3): per mode, with SVR_OPT_EMPTY_SKIP 1 and 0, and render_raycasting beside them.
Per figure: 3 warm-up frames, then the median and the fastest of 5 batches of 10 frames (one synchronisation per batch)."""
import statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from sunvolumerender_amd import abi, host, scenes
name = sys.argv[1] if len(sys.argv) > 1 else "c3"
iso = float(sys.argv[2]) if len(sys.argv) > 2 else 0.15
sc = scenes.make_scene(name)
dev = host.Device(0)
c = host.Canvas(dev, sc.width, sc.height)
scenes.apply_to_canvas(sc, c, 0)


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


c.SetRenderMode(host.Canvas.RENDER_MODE_RAYCASTING)
med, best = timed(c.paint)
print(f"{name} {sc.width}x{sc.height} raycast            : median {med:.3f} ms/frame, fastest {best:.3f}")
for mode, mname in ((abi.PROJ_MIP, "mip"), (abi.PROJ_MEAN, "mean"), (abi.PROJ_ISO, f"iso {iso:g}")):
    for skip in (1, 0):
        dev.set_option(abi.OPT_EMPTY_SKIP, skip)
        dev.set_option(abi.OPT_COUNT, 0)
        med, best = timed(lambda: c.paint_projection(mode, iso=iso))
        dev.set_option(abi.OPT_COUNT, 1); dev.reset_counters(); c.paint_projection(mode, iso=iso, sync=True); cnt = dev.counters()
        dev.set_option(abi.OPT_COUNT, 0)
        print(f"{name} {sc.width}x{sc.height} projection {mname:8s} skip {skip}: median {med:.3f} ms/frame, fastest {best:.3f}  "
              f"steps={cnt['raycast_steps']} taps_executed={cnt['vol_taps_executed']} of {cnt['vol_taps']}")
dev.set_option(abi.OPT_EMPTY_SKIP, 1)
c.close()
