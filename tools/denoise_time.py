#!/usr/bin/env python3
"""Cost of the denoised preview on the GPU: the guide pass (k_guides + the copy of the guides) and the filter + tone map (k_demod +
passes x k_atrous) in ms, wall clock between device synchronisations (includes ~0.02 ms of launch and synchronisation), at several
image sizes.  usage: tools/denoise_time.py [--scenes c3,c3n] [--sizes 512,1024,2048] [--reps 20]"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from sunvolumerender_amd import abi, host, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3,c3n")
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = host.Device(0, fatal_errors=False)
    for name in a.scenes.split(","):
        for n in [int(s) for s in a.sizes.split(",")]:
            sc = scenes.make_scene(name, width=n, height=n)
            cv = host.Canvas(dev, n, n)
            scenes.apply_to_canvas(sc, cv)
            cv.paint_frames(1)
            dev.synchronize()
            guides = dev.malloc(n * n * 32)
            t_g, t_f = [], []
            for r in range(a.reps + 2):
                # the guides are cached: flip the skipping mode (part of the cache key, no effect on the result) to force a rebuild
                dev.set_option(abi.OPT_EMPTY_SKIP, r % 2)
                dev.synchronize()
                t0 = time.perf_counter()
                dev.check(dev.lib.svr_render_guides(C.c_void_p(guides)))
                dev.synchronize()
                t1 = time.perf_counter()
                dev.denoise_to_ldr(cv.img, int(cv.renderParams.hdrBuffer), n, n)
                dev.synchronize()
                t2 = time.perf_counter()
                if r >= 2:
                    t_g.append((t1 - t0) * 1e3)
                    t_f.append((t2 - t1) * 1e3)
            dev.set_option(abi.OPT_EMPTY_SKIP, 1)
            print(f"{name} {n}x{n}: guides with empty-space skipping median {np.median(t_g[1::2]):.3f} ms (min {min(t_g[1::2]):.3f}), "
                  f"without {np.median(t_g[0::2]):.3f} ms; "
                  f"filter {dev.get_denoise_params().passes} passes + tone map median {np.median(t_f):.3f} ms, min {min(t_f):.3f}", flush=True)
            dev.free(guides)
            cv.close()


if __name__ == "__main__":
    main()
