"""Bit-exact pins of the opt-in path-tracer modes (SVR_OPT_LOCAL_MAJORANT, SVR_OPT_ENV_NEE), recorded from this project's own
kernels on an MI355X (tests/golden/make_refactor_pins.py) before the path events and the task prologue of these kernels were moved
into shared helpers (csrc/svr_path.hpp, csrc/svr_tile_tasks.hpp).  The form-to-form tests of tests/test_local_majorant_gpu.py (pools == straight line) cannot see a
change in what the forms SHARE -- lm_step, lm_tentative, the path events of csrc/svr_path.hpp: these fixtures can.

Small frames (48 x 40; 'odd' keeps the 50 x 37 its camera was set up for), float32 accumulators:
  f24: one 24-frame call -- a wave = 2 pixels x 32 frame lanes, 8 of them dead, per-lane whole-ray tests
  f64: one 64-frame call -- a wave = one pixel x 64 frames, shared whole-ray tests
Every local-majorant case in mode 1 (the pool forms) and mode 2 (the straight-line form).  Each file names the commit, the
kernel_source_hash() and the compiler it was recorded with; a failure message repeats them beside today's, so that a compiler
change is told from a code change.  Re-record only when the modes' arithmetic is changed on purpose."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import _build, abi, host, scenes
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
W, H = 48, 40

# (scene, trace depth, SVR_OPT_MACRO_SHIFT_MIN, SVR_OPT_LM_SUBCELLS)
LM_CASES = [("tiny_head", 1, 0, 1),          # 3 lights + env: the record pool
            ("tiny_head", 3, 0, 1),          # the deep pool
            ("tiny_head_noisy", 2, 0, 1),    # half-resolution grid, no empty bit
            ("tiny_bone", 2, 2, 2),          # 4-voxel macro-cells with the sub-cell occupancy forced on: the sub-cell branch of lm_step
            ("odd", 3, 0, 1)]                # clip planes, thin lens, anisotropic spacing
ENV_CASE = ("tiny_head", 3)


def lm_file(name, depth, mode):
    return GOLDEN / f"pin_lm_{name}_d{depth}_m{mode}.npz"


def env_file(name, depth):
    return GOLDEN / f"pin_env_nee_{name}_d{depth}.npz"


def compiler_version():
    try:
        out = subprocess.run([_build._hipcc(), "--version"], capture_output=True, text=True).stdout
        return next((ln.strip() for ln in out.splitlines() if "version" in ln.lower()), "unknown")
    except Exception:
        return "unknown"


def _scene(name, depth):
    if name == "odd":
        from tests.test_more_gpu import _odd_scene
        return _odd_scene(depth=depth)
    return scenes.make_scene(name, trace_depth=depth, width=W, height=H)


def render_pin(dev, name, depth, shift=0, sub=1, lm=0, env_nee=0, frames=(24, 64)):
    """{"f<n>": accumulator after ONE n-frame call of a restarted render} for each n of `frames`"""
    sc = _scene(name, depth)
    canvas = host.Canvas(dev, sc.width, sc.height)
    try:
        dev.set_option(abi.OPT_MACRO_SHIFT_MIN, shift)
        try:
            scenes.apply_to_canvas(sc, canvas)
        finally:
            dev.set_option(abi.OPT_MACRO_SHIFT_MIN, 0)
        dev.set_option(abi.OPT_LOCAL_MAJORANT, lm)
        dev.set_option(abi.OPT_LM_SUBCELLS, sub)
        dev.set_option(abi.OPT_ENV_NEE, env_nee)
        out = {}
        for n in frames:
            canvas.ReStartRender()
            canvas.paint_frames(n, sync=True)
            out[f"f{n}"] = canvas.read_hdr()
        return out
    finally:
        dev.set_option(abi.OPT_LOCAL_MAJORANT, 0)
        dev.set_option(abi.OPT_LM_SUBCELLS, 1)
        dev.set_option(abi.OPT_ENV_NEE, 0)
        canvas.close()


def _check(got, path, what):
    pin = np.load(path)
    origin = (f"{what} (recorded at commit {pin['commit']}, kernel_source_hash {pin['kernel_source_hash']}, {pin['compiler']}; "
              f"now kernel_source_hash {_build.kernel_source_hash()}, {compiler_version()})")
    for key, img in got.items():
        assert pin[key].dtype == np.float32 and pin[key].max() > 0
        assert_bit_exact(img, pin[key], f"{origin}, {key}")


@pytest.mark.parametrize("mode", [1, 2], ids=["pools", "straight_line"])
@pytest.mark.parametrize("name,depth,shift,sub", LM_CASES)
def test_local_majorant_bits_are_the_recorded_ones(hip_dev, name, depth, shift, sub, mode):
    _check(render_pin(hip_dev, name, depth, shift, sub, lm=mode), lm_file(name, depth, mode), f"local majorants, {name} depth {depth} mode {mode}")


def test_env_nee_bits_are_the_recorded_ones(hip_dev):
    """(Holds because the map's sampling table is summed in a fixed order, svr_kernels.hip k_env_mean: with one float atomic per wave the
    table's floor, and one float in 5760 of this frame, moved by an ulp with the order in which the waves arrived.)"""
    name, depth = ENV_CASE
    _check(render_pin(hip_dev, name, depth, env_nee=1, frames=(24,)), env_file(name, depth), f"env NEE, {name} depth {depth}")
