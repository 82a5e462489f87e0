#!/usr/bin/env python3
"""Time the mask calls (svr_region_morph, _combine, _reconstruct, _fill_holes, _detach) on the phantom head: the brain and bone regions
of tools/region_time.py, grown on the device.  Per row the HIP-event time of the call's device work (svr_region_mask_last_ms), median
of 5 calls after a warm-up.  Morph rows: each op at element 6 and 26, radius 1, 2, 4 and 8, with the ratio to the byte floor -- every
unit step reads one mask and writes one, at 8 TB/s, the HBM rate of DESIGN.md section 6.  The time of a call that needs the temporary
(more than one launch) includes its hipMalloc and hipFree.  reconstruct (the brain window's candidates, the seed voxel as marker) is printed next to the grow phase of
svr_region_grow on the same case: the same kernel and sweeps, so the difference is the seed pass over the whole mask.
Every (size, library) pair runs in a child process of its own under its own time limit, so one that goes wrong ends alone; an A/B build
is named by --lib (a library built with SVR_HIP_LIB=<path> SVR_EXTRA_HIPCC_FLAGS=-D... python -m sunvolumerender_amd._build, e.g.
-DSVR_MORPH_ONE_STEP: every unit step a launch of its own, none fused), and the default library is then timed once more after the others, so
that the job shows its own run-to-run spread.
usage: tools/morph_time.py [--n 512] [--lib name=path ...] [--limit SECONDS]"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM = 8e12                                               # bytes / s


def child(n: int, tag: str):
    import numpy as np
    from sunvolumerender_amd import abi, host, scenes

    vox, _ = scenes._volume("head", n)                  # the c3 (512) phantom, without its gradient pass
    dev = host.Device(0)
    lib = dev.lib
    shape = vox.shape
    words = host.region_mask_words(shape)
    mask_bytes = 4 * words
    d_vox = dev.malloc(vox.nbytes)
    dev.to_device(d_vox, vox)
    bufs = {k: dev.malloc(mask_bytes) for k in ("brain", "bone", "cand", "marker", "out")}
    s = n // 48
    bone_at = np.argwhere(vox[n // 2] >= 39321)[0]
    seeds = {"brain": (n // 2, n // 2, n // 2), "bone": (int(bone_at[1]), int(bone_at[0]), n // 2)}
    windows = {"brain": (23593, 28835), "bone": (39321, 65535)}
    st = abi.RegionStats()
    grow_ms = {}
    for name in ("brain", "bone"):
        p = dev.region_params(*windows[name], 6)
        xyz = (C.c_int32 * 3)(*seeds[name])
        phases = []
        for _ in range(6):
            dev.check(lib.svr_region_grow(C.c_void_p(d_vox), n, n, n, 1, xyz, 1, C.byref(p), C.c_void_p(bufs[name]), C.byref(st)))
            ms = [C.c_float(), C.c_float(), C.c_float()]
            lib.svr_region_last_ms(*[C.byref(m) for m in ms])
            phases.append(ms[1].value)
        grow_ms[name] = (statistics.median(phases[1:]), min(phases[1:]), max(phases[1:]), st.sweeps)
        print(f"{tag} {n}^3 {name}: {st.voxels} voxels; svr_region_grow's grow phase {grow_ms[name][0]:.3f} ms ({grow_ms[name][1]:.3f} .. {grow_ms[name][2]:.3f}), "
              f"{st.sweeps} sweeps", flush=True)

    def timed(call, reps=5):
        call()
        t = []
        ms = C.c_float()
        for _ in range(reps):
            call()
            dev.check(lib.svr_region_mask_last_ms(C.byref(ms)))
            t.append(ms.value)
        return statistics.median(t), min(t), max(t)

    out = C.c_void_p(bufs["out"])
    ops = (("dilate", abi.MORPH_DILATE), ("erode", abi.MORPH_ERODE), ("open", abi.MORPH_OPEN), ("close", abi.MORPH_CLOSE))
    for name in ("brain", "bone"):
        src = C.c_void_p(bufs[name])
        for element in (6, 26):
            for opname, op in ops:
                row = {}
                for radius in (1, 2, 4, 8):
                    row[radius] = timed(lambda: dev.check(lib.svr_region_morph(src, n, n, n, op, element, radius, out)))[0]
                steps = 2 if op in (abi.MORPH_OPEN, abi.MORPH_CLOSE) else 1
                floor = {r: steps * r * 2 * mask_bytes / HBM * 1e3 for r in row}
                print(f"{tag} {n}^3 {name:5s} {opname:6s} element {element:2d}: " + "  ".join(f"r{r} {row[r]:7.3f} ms ({row[r] / floor[r]:5.1f} x floor)" for r in row),
                      flush=True)
    a, b = C.c_void_p(bufs["brain"]), C.c_void_p(bufs["bone"])
    for opname, op, nb in (("and", abi.MASK_AND, 2), ("or", abi.MASK_OR, 2), ("andnot", abi.MASK_ANDNOT, 2), ("xor", abi.MASK_XOR, 2), ("not", abi.MASK_NOT, 1)):
        t = timed(lambda: dev.check(lib.svr_region_combine(a, b if nb == 2 else None, n, n, n, op, out)))
        floor = (nb + 1) * mask_bytes / HBM * 1e3
        print(f"{tag} {n}^3 combine {opname:6s}: {t[0]:7.3f} ms ({t[0] / floor:5.1f} x floor)", flush=True)
    for conn in (6, 26):
        t = timed(lambda: dev.check(lib.svr_region_fill_holes(b, n, n, n, conn, 0, out)))
        filled = int(dev.region_stats_of(d_vox, bufs["out"], shape=shape).voxels)
        print(f"{tag} {n}^3 fill_holes bone background {conn:2d}: {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}); {filled} voxels", flush=True)
    seed = (C.c_int32 * 3)(n // 2, n // 2, n // 2 + s)      # the tests' (24, 24, 25), scaled
    status = C.c_int32()
    for element in (6, 26):
        t = timed(lambda: dev.check(lib.svr_region_detach(a, n, n, n, seed, 1, element, 2, 6, 0, out, C.byref(status))))
        kept = int(dev.region_stats_of(d_vox, bufs["out"], shape=shape).voxels)
        print(f"{tag} {n}^3 detach brain element {element:2d} radius 2: {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}); status {status.value}, {kept} voxels", flush=True)
    # reconstruct = the grow phase with masks: the brain window as candidates, the seed voxel as marker
    lo, hi = windows["brain"]
    dev.to_device(bufs["cand"], host.region_mask_pack((vox >= lo) & (vox <= hi)))
    marker = np.zeros(words, dtype=np.uint32)
    x, y, z = seeds["brain"]
    marker[(z * n + y) * ((n + 31) // 32) + (x >> 5)] = 1 << (x & 31)
    dev.to_device(bufs["marker"], marker)
    sweeps = C.c_uint32()
    t = timed(lambda: dev.check(lib.svr_region_reconstruct(C.c_void_p(bufs["marker"]), C.c_void_p(bufs["cand"]), n, n, n, 6, 0, out, C.byref(sweeps))))
    same = np.array_equal(dev.to_host(bufs["out"], (words,), np.uint32), dev.to_host(bufs["brain"], (words,), np.uint32))
    g = grow_ms["brain"]
    print(f"{tag} {n}^3 reconstruct brain: {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}), {sweeps.value} sweeps, mask equal to svr_region_grow's: {same} | "
          f"grow phase of svr_region_grow {g[0]:.3f} ms ({g[1]:.3f} .. {g[2]:.3f}), {g[3]} sweeps", flush=True)
    for ptr in [d_vox, *bufs.values()]:
        dev.free(ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512])
    ap.add_argument("--lib", action="append", default=[], help="name=path of another build to time next to the default one")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a (size, library) pair may take")
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), a.child[1])
        return 0
    libs = [("default", None)] + [tuple(s.split("=", 1)) for s in a.lib] + ([("default-again", None)] if a.lib else [])
    for n in a.n:
        for tag, path in libs:
            env = dict(os.environ)
            if path:
                env["SVR_HIP_LIB"] = str(Path(path).resolve())
            try:
                rc = subprocess.run([sys.executable, __file__, "--child", str(n), tag], env=env, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                print(f"{tag} {n}^3: not finished after {a.limit:.0f} s; stopping here", flush=True)
                return 1
            if rc != 0:
                print(f"{tag} {n}^3: exit status {rc}; stopping here", flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
