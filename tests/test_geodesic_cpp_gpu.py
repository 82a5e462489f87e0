"""examples/render_mhd.cpp -threshold LO HI -split L -largest 1 -keep (the C++ Canvas of include/sunvolumerender/canvas.hpp:
ThresholdRegion, SplitRegion, KeepLargestRegion, ShowRegion) as its own process on the two-ball phantom, against the same steps made of
the Python layer and the numpy references (tests/geodesic_ref.py, tests/label_ref.py) on the volume svr_volume_preprocess leaves on the
device."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import distance_ref as dr
from tests import geodesic_ref as gr
from tests import label_ref as lr
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess
from tests.test_label_cpp_gpu import MEASURED, check_measured
from tests.cpp_example import build_example

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


def test_render_mhd_split_matches_python_and_numpy(hip_dev, tmp_path):
    exe = build_example(tmp_path)
    balls = gr.two_ball_phantom()
    vol = np.where(balls, 1200, -1000).astype(np.int16)
    vol[0, 0, 0] = 2000                                                       # (the window below is the balls alone, not the brightest voxel)
    spacing = (0.8, 0.8, 0.8)
    mhd = write_mhd(tmp_path / "balls.mhd", vol, spacing)
    u16 = _preprocess(hip_dev, vol, spacing)["u16"]                           # what the loader leaves on the device (svr_volume_preprocess)
    value = int(u16[12, 12, 12])
    lo, hi = value - 100, value + 100
    length = 4.96                                                             # a neck radius of 6.2 voxels, in the spacing's units: d2 > 38

    # ---- the same steps in Python, and in numpy.  The C++ Canvas takes the spacing from the float32 members of the volume
    sp = [float(f32(s)) for s in spacing]
    w, unit = host.distance_weights(sp, u16.shape)
    assert w == (256, 256, 256)
    r2 = int(math.floor((length / unit) ** 2))
    steps, step_unit = host.geodesic_weights(sp, 26, u16.shape)
    assert steps == (8, 8, 8, 11, 11, 11, 14) == gr.weights_from_spacing(sp, 26, u16.shape)[0]
    window = hip_dev.region_threshold(u16, lo, hi)
    assert np.array_equal(window, balls)
    cores = dr.ball(balls, dr.ERODE, r2, w)
    assert np.array_equal(cores, dr.ball(balls, dr.ERODE, 38)) and lr.label(cores, 26)[1] == 2
    zones, count, lost, _ = hip_dev.region_split(window, r2, 26, dist_weights=w, step_weights=steps)
    want_zones, want_count, want_lost = gr.split(balls, r2, 26, dist_weights=w, step_weights=steps)
    assert np.array_equal(zones, want_zones) and (count, lost) == (want_count, want_lost) == (2, 0)
    cut = hip_dev.region_zone_cut(zones, 26)
    want_cut = gr.zone_cut(want_zones, 26)
    assert np.array_equal(cut, want_cut) and lr.label(want_cut, 26)[1] == 2
    want_largest, kept = lr.select_by_size(*lr.label(want_cut, 26), 0, 1)
    assert kept == 1 and 0 < want_largest.sum() < want_cut.sum() < balls.sum()

    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", "64", "48", "-threshold", str(lo), str(hi), "-conn", "26", "-split", str(length),
                          "-largest", "1", "-keep", "-o", str(tmp_path / "split.tga")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    m = re.search(rf"threshold window {lo}\.\.{hi} conn 26: (\d+) parts, " + MEASURED, res.stdout)
    assert m and int(m.group(1)) == 1, res.stdout
    check_measured(m, 2, u16, balls, spacing)
    m = re.search(r"split ([0-9.e+-]+) conn 26: (\d+) parts, " + MEASURED, res.stdout)
    assert m and res.stdout.index("split ") > res.stdout.index("threshold window"), res.stdout
    assert float(m.group(1)) == pytest.approx(length, rel=1e-5) and int(m.group(2)) == 2
    check_measured(m, 3, u16, want_cut, spacing)
    m = re.search(r"largest 1 conn 26: (\d+) of (\d+) parts kept, " + MEASURED, res.stdout)
    assert m and res.stdout.index("largest 1") > res.stdout.index("split "), res.stdout
    assert (int(m.group(1)), int(m.group(2))) == (1, 2)
    check_measured(m, 3, u16, want_largest, spacing)
    assert "cleaned (" not in res.stdout                                       # that line belongs to the steps that had it
