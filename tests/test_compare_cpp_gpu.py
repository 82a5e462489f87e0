"""examples/render_mhd.cpp -compare-mask FILE (the C++ Canvas of include/sunvolumerender/canvas.hpp: CompareRegionWithFile, CompareRegion)
as its own process: a window's mask is saved by one run, a second run compares the same window of the median-filtered volume with that
file, and the printed line must be what the Python layer measures for the same two masks under the weights of the file's spacing."""
import re
import subprocess

import numpy as np
import pytest

from sunvolumerender_amd import host, scenes
from tests import compare_ref as cr
from tests.cpp_example import build_example
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess

pytestmark = pytest.mark.gpu
f32 = np.float32
FLOAT = r"([0-9.e+-]+|nan)"


def test_render_mhd_compare_mask_matches_python(hip_dev, tmp_path):
    exe = build_example(tmp_path)
    v = scenes.make_ct_head_volume(48)[:28, :36, :44].astype(np.float64)
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000
    spacing = (0.9, 0.9, 1.5)
    mhd = write_mhd(tmp_path / "ct.mhd", vol, spacing)
    u16 = _preprocess(hip_dev, vol, spacing)["u16"]                           # what the loader leaves on the device (svr_volume_preprocess)
    lo, hi = (int(t) for t in np.percentile(u16[u16 > 0], [40, 80]))
    W, H = 64, 48
    saved = tmp_path / "m.mhd"

    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-threshold", str(lo), str(hi), "-save-mask", str(saved), "-o",
                          str(tmp_path / "a.tga")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-median", "18", "1", "-threshold", str(lo), str(hi), "-compare-mask",
                          str(saved), "-o", str(tmp_path / "b.tga")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    m = re.search(rf"compare-mask: dice {FLOAT} jaccard {FLOAT} hd {FLOAT} hd95 {FLOAT} assd {FLOAT} mm \(both (\d+), region only (\d+), file only (\d+) voxels\)",
                  res.stdout)
    assert m, res.stdout

    # the same in Python: A = the window of the filtered volume (the region), B = the window of the volume (the file)
    a = hip_dev.region_threshold(hip_dev.volume_median(u16, 18, 1), lo, hi)
    b = hip_dev.region_threshold(u16, lo, hi)
    assert (a ^ b).any() and (a & b).any()
    weights, unit = host.distance_weights([float(f32(s)) for s in spacing], u16.shape)      # the Canvas keeps the spacing as float32
    c = hip_dev.region_compare(a, b, 6, weights)
    want = cr.compare(a, b, 6, weights)
    assert cr.comparison_of_struct(c) == want
    assert [int(g) for g in m.groups()[5:]] == want["overlap"][:3]
    meas = host.compare_measure(c, unit)
    assert [float(g) for g in m.groups()[:5]] == [meas.dice, meas.jaccard, meas.hausdorff, meas.hausdorff_q, meas.assd]       # %.17g round-trips
    assert 0.0 < meas.dice < 1.0 and meas.hausdorff >= meas.hausdorff_q >= 0.0 and meas.hausdorff > 0.0 and meas.assd > 0.0

    # a mask of other dimensions, and a file that is no mask, are refused
    other = write_mhd(tmp_path / "small.mhd", np.zeros((4, 4, 4), np.uint8), spacing)
    for bad in (other, mhd):
        res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-threshold", str(lo), str(hi), "-compare-mask", str(bad), "-o",
                              str(tmp_path / "c.tga")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 1 and "-compare-mask" in res.stderr, res.stdout + res.stderr
    res = subprocess.run([str(exe), str(mhd), "-compare-mask", str(saved)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "needs -grow" in res.stderr
