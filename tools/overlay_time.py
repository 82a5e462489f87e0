#!/usr/bin/env python3
"""Time the overlay calls on a scene (default c3): svr_slice_ids, svr_overlay_ids, the two in a row and the fused svr_overlay_slice for an
axial plane, an oblique slab of 32 samples and a 256-slice axial stack, each beside svr_render_slice / svr_render_slice_stack for the same
params in the same process; and the 3D chain (svr_render_hits, svr_hit_ids, svr_overlay_ids) beside render_raycasting.  The sources are
the mask of the brain window and the zones of its split (svr_region_split, ball r2 = 16, connectivity 26).
Per figure: 3 warm-up calls, then the median and the fastest of 5 batches of calls (10 per batch, 2 for the stack), wall clock around work
that ends in one synchronisation per batch.  The fused call and the two-call form of the stack are also timed against each other in
alternating batches, which is the comparison that decides whether the fused call earns its place.  The lines go to stdout and to --out.
usage: tools/overlay_time.py [scene] [--count 256] [--out profiles/overlay_times.txt]"""
import argparse
import builtins
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np

from sunvolumerender_amd import abi, host, scenes

ap = argparse.ArgumentParser()
ap.add_argument("scene", nargs="?", default="c3")
ap.add_argument("--count", type=int, default=256)
ap.add_argument("--out", default=str(ROOT / "profiles" / "overlay_times.txt"))
args = ap.parse_args()
open(args.out, "w").close()


def print(*a, **kw):                                    # every line goes to stdout and to the record
    builtins.print(*a, **kw, flush=True)
    with open(args.out, "a") as f:
        builtins.print(*a, file=f)


BRAIN = (23593, 28835)
SPLIT_R2 = 16
sc = scenes.make_scene(args.scene)
dev = host.Device(0)
lib = dev.lib
c = host.Canvas(dev, sc.width, sc.height)
scenes.apply_to_canvas(sc, c, 0)
W, H, count = sc.width, sc.height, args.count
nz, ny, nx = shape = sc.vox.shape
tag = f"{args.scene} {W}x{H}"
print(f"# {dev.info()}; {tag}, volume {nx} x {ny} x {nz}")

# the sources: the brain window and the zones of its split
d_vox = dev.malloc(sc.vox.nbytes)
dev.to_device(d_vox, sc.vox)
d_mask = dev.malloc(4 * host.region_mask_words(shape))
d_zones = dev.malloc(4 * sc.vox.size)
dev.check(lib.svr_region_threshold(C.c_void_p(d_vox), nx, ny, nz, 1, BRAIN[0], BRAIN[1], None, None, C.c_void_p(d_mask)))
_, parts, lost, _ = dev.region_split(d_mask, SPLIT_R2, 26, shape=shape, out_ptr=d_zones)
dev.free(d_vox)
print(f"# sources: the brain window {BRAIN}, and the {parts} zones of its split (r2 {SPLIT_R2}, connectivity 26, {lost} voxels unreached)")
SOURCES = (("mask", dict(mask=d_mask)), ("labels", dict(labels=d_zones)))

d_imgs = dev.malloc(4 * W * H * count)
d_ids = dev.malloc(4 * W * H * count)
style = dev.overlay_style()


def timed(call, warm=3, batches=5, n=10):
    for _ in range(warm):
        call()
    dev.synchronize()
    ms = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        dev.synchronize()
        ms.append((time.perf_counter() - t0) / n * 1e3)
    return statistics.median(ms), min(ms)


def alternating(a, b, rounds=7, n=2):
    """medians of a and b, timed in alternating batches"""
    ta, tb = [], []
    for call, t in ((a, None), (b, None)):
        call()
    dev.synchronize()
    for _ in range(rounds):
        for call, t in ((a, ta), (b, tb)):
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            dev.synchronize()
            t.append((time.perf_counter() - t0) / n * 1e3)
    return statistics.median(ta), statistics.median(tb)


def row(what, med, best, unit="ms"):
    print(f"{tag} {what:58s}: median {med:8.3f} {unit}, fastest {best:8.3f}")


# ---- slices
axial = c.slice_params_axis(2, 0.47)
voxel = float(sc.spacing[0])
ext = max(d * s for d, s in zip(sc.dim, sc.spacing))
px = 1.2 * ext / W
a, b = np.array([np.sqrt(2.0), 1.0 / np.pi, -np.sqrt(3.0) / 2]), np.array([np.e / 7, -np.sqrt(5.0), 0.37])
a /= np.linalg.norm(a); b -= a * np.dot(a, b); b /= np.linalg.norm(b)
oblique = abi.SliceParams.from_buffer_copy(axial)
oblique.center = abi.vec3(0.0, 0.0, 0.0)
oblique.u, oblique.v = abi.vec3(*(px * a)), abi.vec3(*(px * b))
oblique.thickness, oblique.step, oblique.mode = 31.0 * voxel, voxel, abi.SLAB_MIP
first, last = c.slice_params_axis(2, 0.0), c.slice_params_axis(2, 1.0)
spacing = -(last.center.z - first.center.z) / max(count - 1, 1)          # n = -z for axis 2
decision = []
for cname, p, n_slices, sp, reps in (("axial plane", axial, 1, 0.0, 10), ("oblique slab 32", oblique, 1, 0.0, 10),
                                     (f"stack of {count} axial", first, count, spacing, 2)):
    def render():
        dev.check(lib.svr_render_slice_stack(C.c_void_p(d_imgs), C.byref(c.deviceVolume), C.byref(c.transferFunction), W, H, C.byref(p), n_slices,
                                             C.c_float(sp)))
    row(f"{cname}: svr_render_slice" + ("_stack" if n_slices > 1 else ""), *timed(render, n=reps))
    for sname, src in SOURCES:
        def ids():
            dev.slice_ids(d_ids, c.deviceVolume, shape, W, H, p, count=n_slices, spacing=sp, **src)

        def blend():
            dev.overlay_ids(d_imgs, d_ids, W, H, n_slices, style)

        def two():
            ids(); blend()

        def fused():
            dev.overlay_slice(d_imgs, c.deviceVolume, shape, W, H, p, style=style, count=n_slices, spacing=sp, **src)

        render(); ids(); dev.synchronize()
        marked = int(np.count_nonzero(dev.to_host(d_ids, (H, W), np.uint32)))
        row(f"{cname}, {sname}: svr_slice_ids ({marked} px of slice 0 marked)", *timed(ids, n=reps))
        row(f"{cname}, {sname}: svr_overlay_ids", *timed(blend, n=reps))
        row(f"{cname}, {sname}: svr_slice_ids + svr_overlay_ids", *timed(two, n=reps))
        row(f"{cname}, {sname}: svr_overlay_slice (fused)", *timed(fused, n=reps))
        t2, tf = alternating(two, fused, n=reps)
        print(f"{tag} {cname}, {sname}: alternating batches: two calls {t2:.3f} ms, fused {tf:.3f} ms: fused / two calls = {tf / t2:.2f}")
        if n_slices > 1:
            decision.append((sname, t2, tf))

# ---- the 3D chain
d_hits = dev.malloc(W * H * host.HIT_DTYPE.itemsize)
c.SetRenderMode(host.Canvas.RENDER_MODE_RAYCASTING)
row("3D: render_raycasting", *timed(lambda: c.paint()))
hp = abi.HitParams(abi.HIT_OPACITY, 0.5, 0.5)


def hits():
    dev.check(lib.svr_render_hits(C.c_void_p(d_hits), C.byref(c.deviceVolume), C.byref(c.transferFunction), C.byref(c.camera), C.c_float(c.stepSize),
                                  C.byref(hp)))


row("3D: svr_render_hits opacity 0.5", *timed(hits))
for sname, src in SOURCES:
    def hit_ids():
        dev.hit_ids(d_ids, d_hits, W, H, c.deviceVolume, shape, **src)

    def blend():
        dev.overlay_ids(c.img, d_ids, W, H, 1, style)

    def chain():
        hits(); hit_ids(); blend()

    row(f"3D, {sname}: svr_hit_ids", *timed(hit_ids))
    row(f"3D, {sname}: svr_overlay_ids", *timed(blend))
    row(f"3D, {sname}: svr_render_hits + svr_hit_ids + svr_overlay_ids", *timed(chain))

for sname, t2, tf in decision:
    print(f"# the stack, {sname}: fused {tf:.3f} ms against {t2:.3f} ms for the two calls: the fused call {'beats' if tf < t2 else 'DOES NOT beat'} them")
for p in (d_hits, d_imgs, d_ids, d_mask, d_zones):
    dev.free(p)
c.close()
