#!/usr/bin/env python3
"""What the noise estimate costs and what render-until-converged needs.

Default: per image size, a render with SVR_OPT_NOISE_ESTIMATE on through the checkpoints 8, 16 ... --frames (each runs the fused estimate +
snapshot kernel once: time it with `rocprofv3 --kernel-trace --stats -- python tools/noise_time.py`), the estimates it reports, and the wall
time of svr_estimate_noise (the plain kernel + the tile sum + one stream synchronisation) over --reps calls.
--until T1,T2,...: per scene, the frames and wall time of svr_render_pathtracer_until (Canvas.paint_until, the call render_mhd -noise makes)
for each target, from a restart, capped at --frames.
usage: tools/noise_time.py [--scene c3] [--sizes 1024,2048] [--frames 256] [--reps 50] [--until 0.01,0.005 --scenes c3,c3n,c3b]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from sunvolumerender_amd import host, scenes  # noqa: E402


def checkpoints(dev, name, size, frames, reps):
    sc = scenes.make_scene(name, width=size, height=size)
    cv = host.Canvas(dev, size, size)
    scenes.apply_to_canvas(sc, cv)
    try:
        cv.SetNoiseEstimate(True)
        cv.ReStartRender()
        k = 4
        while cv.renderParams.frameNo + k <= frames:
            cv.paint_frames(k)
            k = cv.renderParams.frameNo
            e = cv.noise_estimate()
            if e.frames:
                print(f"{name} {size}x{size}: estimate at {e.frames} frames (against {e.frames_ref}): rmse {e.rmse:.5f}, largest tile "
                      f"{e.tile_max:.5f}, {e.pixels} pixels, {e.nonfinite} non-finite", flush=True)
        cv.SetNoiseEstimate(False)
        dev.synchronize()
        nbytes = size * size * 12
        ref = dev.malloc(nbytes)
        try:
            dev.to_device(ref, cv.read_hdr())
            hdr = int(cv.renderParams.hdrBuffer)
            t = []
            for r in range(reps + 3):
                t0 = time.perf_counter()
                dev.estimate_noise(ref, 4, hdr, 8, size, size)
                if r >= 3:
                    t.append((time.perf_counter() - t0) * 1e6)
        finally:
            dev.free(ref)
        print(f"{name} {size}x{size}: svr_estimate_noise (24 B per pixel read, tile sum, one synchronisation) median {np.median(t):.1f} us, "
              f"min {min(t):.1f} us over {reps} calls", flush=True)
    finally:
        cv.close()


def until(dev, name, targets, frames, depth):
    sc = scenes.make_scene(name, trace_depth=depth)
    cv = host.Canvas(dev, sc.width, sc.height)
    scenes.apply_to_canvas(sc, cv)
    try:
        cv.paint_frames(8)                       # warm-up: acceleration data, queues
        dev.synchronize()
        for tgt in targets:
            cv.ReStartRender()
            dev.synchronize()
            t0 = time.perf_counter()
            k = cv.paint_until(tgt, max_frames=frames)
            dev.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            e = cv.noise_estimate()
            print(f"{name} depth {depth} {sc.width}x{sc.height}: target {tgt:g}: {k} frames in {ms:.1f} ms; estimate at {e.frames} frames: "
                  f"rmse {e.rmse:.5f}, largest tile {e.tile_max:.5f}", flush=True)
    finally:
        cv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3")
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--until", default="")
    ap.add_argument("--scenes", default="c3,c3n,c3b")
    ap.add_argument("--depth", type=int, default=1)
    a = ap.parse_args()
    dev = host.Device(0, fatal_errors=False)
    if a.until:
        for name in a.scenes.split(","):
            until(dev, name, [float(t) for t in a.until.split(",")], a.frames, a.depth)
        return
    for n in [int(s) for s in a.sizes.split(",")]:
        checkpoints(dev, a.scene, n, a.frames, a.reps)


if __name__ == "__main__":
    main()
