#!/usr/bin/env python3
"""Parameter sweep of the denoised preview (svr_denoise_params): for each scene and spp, the RMSE of the tone-mapped image against a
4 096-spp render (denoised / raw) and the mean luminance over O > 0 pixels against the reference.  Prints one line per setting.
usage: tools/denoise_sweep.py [--scenes small_head,c3] [--spp 1,4] [--ref-spp 4096] [--grid quick|full]"""
import argparse
import itertools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from sunvolumerender_amd import host, scenes  # noqa: E402

LUM = np.array([0.2126, 0.7152, 0.0722])


def tm(hdr, exposure):
    return np.clip(1.0 - np.exp(-np.asarray(hdr, np.float64) * 16.0 * exposure), 0, None) ** 2.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="small_head,c3")
    ap.add_argument("--depths", default="1")
    ap.add_argument("--spp", default="1,4")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--grid", default="quick")
    a = ap.parse_args()
    dev = host.Device(0, fatal_errors=False)
    if a.grid == "full":
        grid = dict(sigma_depth=[0.5, 1.0, 2.0], sigma_normal=[8.0, 32.0, 128.0], sigma_albedo=[0.05, 0.1, 0.2, 0.4], sigma_opacity=[0.05, 0.2, 0.8],
                    passes=[4, 5])
    else:
        grid = dict(sigma_depth=[0.5, 1.0, 2.0], sigma_normal=[8.0, 32.0], sigma_albedo=[0.1, 0.2, 0.4], sigma_opacity=[0.1, 0.2, 0.8], passes=[5])
    keys = list(grid)
    for name in a.scenes.split(","):
        for depth in [int(d) for d in a.depths.split(",")]:
            sc = scenes.make_scene(name, trace_depth=depth)
            cv = host.Canvas(dev, sc.width, sc.height)
            scenes.apply_to_canvas(sc, cv)
            cv.ReStartRender()
            for _ in range(a.ref_spp // 64):
                cv.paint_frames(64)
            dev.synchronize()
            ref = cv.read_hdr().astype(np.float64)
            fg = cv.read_guides()[..., 7] > 0
            out = dev.malloc(cv.W * cv.H * 12)
            for spp in [int(s) for s in a.spp.split(",")]:
                cv.ReStartRender()
                cv.paint_frames(spp)
                dev.synchronize()
                raw = cv.read_hdr().astype(np.float64)
                ok = np.isfinite(raw).all(-1) & np.isfinite(ref).all(-1)
                e_raw = np.sqrt(np.mean((tm(raw[ok], sc.exposure) - tm(ref[ok], sc.exposure)) ** 2))
                m_ref = float((ref[fg & ok] @ LUM).mean())
                m_raw = float((raw[fg & ok] @ LUM).mean())
                print(f"# {name} depth {depth} {spp} spp: raw RMSE {e_raw:.5f}, raw mean lum {100 * (m_raw / m_ref - 1):+.2f} % of the reference", flush=True)
                for vals in itertools.product(*(grid[k] for k in keys)):
                    p = dev.denoise_params(**dict(zip(keys, vals)))
                    dev.denoise_hdr(out, int(cv.renderParams.hdrBuffer), cv.W, cv.H, p)
                    den = dev.to_host(out, (cv.H, cv.W, 3), np.float32).astype(np.float64)
                    okd = ok & np.isfinite(den).all(-1)
                    e = np.sqrt(np.mean((tm(den[okd], sc.exposure) - tm(ref[okd], sc.exposure)) ** 2))
                    m = float((den[fg & okd] @ LUM).mean())
                    print(f"{name} d{depth} {spp}spp " + " ".join(f"{k}={v}" for k, v in zip(keys, vals)) +
                          f" ratio {e / e_raw:.4f} mean {100 * (m / m_ref - 1):+.2f} %", flush=True)
            dev.free(out)
            cv.close()


if __name__ == "__main__":
    main()
