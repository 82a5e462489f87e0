#!/usr/bin/env python3
"""What adaptive sampling saves: per scene and tile target T, svr_render_pathtracer_until with the tile target alone (Canvas.paint_until(0,
tile_target=T): every pixel traced until the worst tile meets T) against svr_render_pathtracer_adaptive (Canvas.paint_adaptive(T): tiles
freeze one by one), both from a restart and capped at --frames: wall time, samples traced, the share of tiles frozen at each checkpoint and
the final largest tile RMSE.  Time the kernels (trace, masked estimate) with `rocprofv3 --kernel-trace --stats -- python tools/adaptive_time.py`.
usage: tools/adaptive_time.py [--scenes c3,c3n,c3b] [--targets 0.02,0.01] [--frames 4096] [--depth 1] [--reps 2]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from sunvolumerender_amd import host, scenes  # noqa: E402


def run(dev, name, targets, frames, depth, reps):
    sc = scenes.make_scene(name, trace_depth=depth)
    cv = host.Canvas(dev, sc.width, sc.height)
    scenes.apply_to_canvas(sc, cv)
    px = sc.width * sc.height
    try:
        cv.paint_frames(8)                       # warm-up: acceleration data, queues
        dev.synchronize()
        for tgt in targets:
            t_u, t_a = [], []
            for _ in range(reps):
                cv.ReStartRender()
                dev.synchronize()
                t0 = time.perf_counter()
                k = cv.paint_until(0.0, tile_target=tgt, max_frames=frames)
                dev.synchronize()
                t_u.append((time.perf_counter() - t0) * 1e3)
                e = cv.noise_estimate()
                cv.ReStartRender()
                dev.synchronize()
                t0 = time.perf_counter()
                r = cv.paint_adaptive(tgt, 0, frames)
                dev.synchronize()
                t_a.append((time.perf_counter() - t0) * 1e3)
            fr, _ = cv.adaptive_tiles()
            share = {int(c): round(float((fr == c).mean()), 4) for c in np.unique(fr)}
            print(f"{name} depth {depth} {sc.width}x{sc.height} T {tgt:g}: until {k} frames, {px * k} samples, {min(t_u):.1f} ms, largest tile "
                  f"{e.tile_max:.5f} | adaptive {r.frames_min}..{r.frames_max} frames, {r.pixel_frames} samples ({r.pixel_frames / (px * k):.3f}), "
                  f"{min(t_a):.1f} ms ({min(t_a) / min(t_u):.3f}), {r.checkpoints} estimates, {r.tiles_active} tiles active at the end, largest "
                  f"tile {r.tile_max:.5f}, rmse {r.rmse:.5f}; tiles by frame count {share}", flush=True)
    finally:
        cv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3,c3n,c3b")
    ap.add_argument("--targets", default="0.02,0.01")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    dev = host.Device(0, fatal_errors=False)
    for name in a.scenes.split(","):
        run(dev, name, [float(t) for t in a.targets.split(",")], a.frames, a.depth, a.reps)


if __name__ == "__main__":
    main()
