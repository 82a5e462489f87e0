#!/usr/bin/env python3
"""Phase profile of the lane machine (experiment build: SVR_EXTRA_HIPCC_FLAGS=-DSVR_TEST_HOOKS SVR_HIP_LIB=<path> python -m sunvolumerender_amd._build).
usage: SVR_HIP_LIB=... tools/phase_prof.py [--scene c3] [--depth 4] [--frames 32] setting..."""
import argparse, ctypes as C, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from sunvolumerender_amd import abi, host, scenes  # noqa: E402
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="c3"); ap.add_argument("--depth", type=int, default=4); ap.add_argument("--frames", type=int, default=32)
ap.add_argument("settings", nargs="*", default=["queue=2"])
a = ap.parse_args()
sc = scenes.make_scene(a.scene, trace_depth=a.depth)
dev = host.Device(0, fatal_errors=False)
c = host.Canvas(dev, sc.width, sc.height)
scenes.apply_to_canvas(sc, c)
names = ["primary", "refill", "shade", "cheap", "fetch", "march", "end", "fold"]
fn = dev.lib.svr_debug_phase_profile
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
for setting in a.settings:
    for kv in filter(None, setting.split(",")):
        k, v = kv.split("=")
        dev.set_option(getattr(abi, "OPT_" + k.upper()), int(v))
    c.ReStartRender(); c.paint_frames(a.frames); dev.synchronize()
    dev.reset_counters()
    c.ReStartRender()
    t0 = time.perf_counter(); c.paint_frames(a.frames); dev.synchronize(); dt = time.perf_counter() - t0
    out = np.zeros(32, dtype=np.uint64)
    fn(out.ctypes.data_as(C.c_void_p), 32)
    tot = float(sum(out[2 * i] for i in range(8)))
    print(f"== {a.scene} depth {a.depth} {setting}: {dt / a.frames * 1e3:.4f} ms/frame; wave-cycles by phase (share, lane utilisation)")
    for i, n in enumerate(names):
        cyc, lc = float(out[2 * i]), float(out[2 * i + 1])
        if cyc:
            print(f"   {n:8s} {cyc / tot * 100:6.2f} %   util {lc / cyc / 64 * 100:5.1f} %")
    # the tile kernel's task loop (svr_lanes.hpp: PH_TICKET = 9, PH_LOOP = 10): the waves' whole loops, and their waits for a ticket's value
    loop, ticket = float(out[20]), float(out[18])
    if loop:
        print(f"   task loop {loop:.4g} wave-cycles = 100 %: ticket wait {ticket / loop * 100:.2f} %, " +
              ", ".join(f"{n} {float(out[2 * i]) / loop * 100:.2f} %" for i, n in enumerate(names) if out[2 * i]) +
              f", unstamped {(loop - ticket - tot) / loop * 100:.2f} %")
    # the shadow-walk iterations that run in place in the task loop (PH_FIRST = 11), stamped apart from the machine's cheap rounds, and behind the
    # phases (words 24, 25) the shaded events that have a shadow walk and the records pushed for them
    if out[22]:
        print(f"   first (in place) {float(out[22]) / (loop or tot) * 100:.2f} % of the {'task loop' if loop else 'stamped phases'}   util {float(out[23]) / float(out[22]) / 64 * 100:5.1f} %")
    if out[24]:
        print(f"   shadow walks {int(out[24])}, records pushed {int(out[25])} = {float(out[25]) / float(out[24]) * 100:.2f} %   ({int(out[24]) / a.frames:.0f} / {int(out[25]) / a.frames:.0f} per frame)")
    # the whole-ray march that the pixels of a pair share (svr_walk.hpp, walk_setup_shared; words 26 .. 29): tasks that marched for the pair, reused
    # the kept march, were refused by it (and marched alone), marched alone because their own lanes would not pass against the pair's reference
    if any(out[26:30]):
        sh, re_, rf, al = (int(v) for v in out[26:30])
        tot_m = sh + re_ + rf + al
        print(f"   shared march: {tot_m} tasks with a hit lane: marched for the pair {sh}, reused {re_} = {re_ / tot_m * 100:.1f} %, refused {rf}, alone {al}"
              f"   -> {(sh + rf + al) / tot_m:.3f} marches per task")
    if out[16]:
        if a.depth > 1:
            print(f"   cheap-loop iterations {int(out[16])}, mean walking lanes {float(out[17]) / float(out[16]):.1f}")
        else:
            print(f"   primary walks (count=1 only): executed lane-iterations / (64 x longest walk of the wave) = {float(out[17]) / float(out[16]):.3f}")
c.close()
