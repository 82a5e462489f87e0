#!/usr/bin/env python3
"""Time svr_render_slice / svr_render_slice_stack on a scene (default c3): an axial plane, an oblique plane, an oblique slab of 32
samples in the three modes, each with SVR_OPT_EMPTY_SKIP 1 and 0, and a 256-slice axial stack as one call against 256 calls;
render_raycasting and svr_render_projection MIP are timed in the same process as the yardstick.
Per figure: 3 warm-up calls, then the median and the fastest of 5 batches of 10 calls (one synchronisation per batch)."""
import ctypes as C
import statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
from sunvolumerender_amd import abi, host, scenes
name = sys.argv[1] if len(sys.argv) > 1 else "c3"
sc = scenes.make_scene(name)
print(f"# {name}: volume ready", flush=True)
dev = host.Device(0)
c = host.Canvas(dev, sc.width, sc.height)
scenes.apply_to_canvas(sc, c, 0)
tag = f"{name} {sc.width}x{sc.height}"


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


def counted(paint):
    dev.set_option(abi.OPT_COUNT, 1); dev.reset_counters(); paint(); dev.synchronize(); cnt = dev.counters()
    dev.set_option(abi.OPT_COUNT, 0)
    return cnt


c.SetRenderMode(host.Canvas.RENDER_MODE_RAYCASTING)
med, best = timed(c.paint)
print(f"{tag} raycast                      : median {med:.3f} ms, fastest {best:.3f}", flush=True)
med, best = timed(lambda: c.paint_projection(abi.PROJ_MIP))
print(f"{tag} projection mip               : median {med:.3f} ms, fastest {best:.3f}", flush=True)

axial = c.slice_params_axis(2, 0.47)
voxel = float(sc.spacing[0])
ext = max(d * s for d, s in zip(sc.dim, sc.spacing))
px = 1.2 * ext / sc.width
a, b = np.array([np.sqrt(2.0), 1.0 / np.pi, -np.sqrt(3.0) / 2]), np.array([np.e / 7, -np.sqrt(5.0), 0.37])
a /= np.linalg.norm(a); b -= a * np.dot(a, b); b /= np.linalg.norm(b)
oblique = abi.SliceParams.from_buffer_copy(axial)
oblique.center = abi.vec3(0.0, 0.0, 0.0)
oblique.u, oblique.v = abi.vec3(*(px * a)), abi.vec3(*(px * b))
cases = [("axial plane", axial, {}), ("oblique plane", oblique, {})]
for mode, mname in ((abi.SLAB_MIP, "mip"), (abi.SLAB_MINIP, "minip"), (abi.SLAB_MEAN, "mean")):
    cases.append((f"oblique slab 32 {mname}", oblique, dict(thickness=31.0 * voxel, step=voxel, mode=mode)))
cases.append(("oblique slab 256 mip", oblique, dict(thickness=255.0 * voxel, step=voxel, mode=abi.SLAB_MIP)))
cases.append(("oblique slab 256 mean", oblique, dict(thickness=255.0 * voxel, step=voxel, mode=abi.SLAB_MEAN)))
for cname, p, kw in cases:
    for skip in (1, 0):
        dev.set_option(abi.OPT_EMPTY_SKIP, skip)
        med, best = timed(lambda: c.paint_slice(p, **kw))
        cnt = counted(lambda: c.paint_slice(p, **kw))
        print(f"{tag} slice {cname:22s} skip {skip}: median {med:.3f} ms, fastest {best:.3f}  "
              f"samples={cnt['raycast_steps']} taps_executed={cnt['vol_taps_executed']} of {cnt['vol_taps']}", flush=True)
dev.set_option(abi.OPT_EMPTY_SKIP, 1)

# a 256-slice axial stack across the volume: one call against 256 calls
count = 256
first = c.slice_params_axis(2, 0.0)
last = c.slice_params_axis(2, 1.0)
spacing = -(last.center.z - first.center.z) / (count - 1)          # n = -z for axis 2
buf = dev.malloc(count * sc.width * sc.height * 4)
med, best = timed(lambda: c.paint_slice_stack(buf, first, count, spacing), batches=5, n=2)
print(f"{tag} stack of {count} axial, one call : median {med:.3f} ms, fastest {best:.3f}", flush=True)
singles = []
for k in range(count):
    p = abi.SliceParams.from_buffer_copy(first)
    p.center.z = first.center.z - spacing * k
    singles.append(p)
img = c.img


def one_by_one():
    for k, p in enumerate(singles):
        c.img = buf + k * sc.width * sc.height * 4
        c.paint_slice(p)
    c.img = img


med, best = timed(one_by_one, batches=5, n=2)
print(f"{tag} stack of {count} axial, {count} calls: median {med:.3f} ms, fastest {best:.3f}", flush=True)
dev.free(buf)
c.close()
