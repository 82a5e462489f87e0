"""examples/render_mhd.cpp -fill-between (the C++ Canvas of include/sunvolumerender/canvas.hpp: FillRegionBetweenSlices, and through it
RegionDistanceUnits' weights) as its own process, on a MetaImage that holds only every fourth axial slice of the head: the mask it saves
must be the numpy reference's (tests/fillbetween_ref.py) and the line it prints must say what the reference counts."""
import re
import subprocess

import numpy as np
import pytest

from sunvolumerender_amd import host, io, scenes
from tests import fillbetween_ref as fr
from tests.cpp_example import build_example
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess

pytestmark = pytest.mark.gpu
f32 = np.float32


def test_render_mhd_fill_between_matches_the_reference(hip_dev, tmp_path):
    exe = build_example(tmp_path)
    v = scenes.make_ct_head_volume(48)[:29, :36, :44].astype(np.float64)
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000
    full = vol.copy()
    vol[np.arange(vol.shape[0]) % 4 != 0] = -1000                             # three slices of four are air
    spacing = (0.8, 1.2, 1.5)                                                 # in-plane weights that differ
    mhd = write_mhd(tmp_path / "sparse.mhd", vol, spacing)
    u16 = _preprocess(hip_dev, vol, spacing)["u16"]                           # what the loader leaves on the device (svr_volume_preprocess)
    lo, hi = (int(t) for t in np.percentile(u16[u16 > 0], [40, 100]))
    window = hip_dev.region_threshold(u16, lo, hi)
    assert window[::4].any() and not window[np.arange(window.shape[0]) % 4 != 0].any()
    w, _ = host.distance_weights([float(f32(s)) for s in spacing], u16.shape)  # the C++ Canvas takes the spacing from the float32 members of the volume
    assert w[0] != w[1]
    base = [str(exe), str(mhd), "-raycast", "-size", "32", "24", "-threshold", str(lo), str(hi)]

    def run(*args):
        saved = tmp_path / "m.mhd"
        res = subprocess.run(base + list(args) + ["-save-mask", str(saved), "-o", str(tmp_path / "a.tga")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        print(res.stdout)
        got, _ = io.mhd_read(str(saved))
        return got.astype(bool), res.stdout

    got, text = run("-fill-between", "z")
    want, info = fr.fill_between(window, 2, weights=w)
    assert np.array_equal(got, want)
    assert np.array_equal(hip_dev.region_fill_between(window, 2, weights=w)[0], want)
    assert info["gaps"] >= 5 and info["voxels_out"] > 2 * info["voxels_in"]
    m = re.search(r"fill-between z: (\d+) keys \((\d+) \.\. (\d+)\), (\d+) gaps, (\d+) slices filled, (\d+) -> (\d+) voxels, volume", text)
    assert m and [int(t) for t in m.groups()] == [info[k] for k in ("keys", "first_key", "last_key", "gaps", "filled_slices", "voxels_in", "voxels_out")], text
    assert text.index("fill-between z") > text.index("threshold window")
    # nearer to the window of the volume that has all its slices than the sparse mask is
    truth = hip_dev.region_threshold(_preprocess(hip_dev, full, spacing)["u16"], lo, hi)
    assert fr.dice(got, truth) > fr.dice(window, truth)

    # along y every slice holds a voxel: every slice is a key, there is no gap, and the mask stays
    got, text = run("-fill-between", "y")
    assert np.array_equal(got, window)
    assert re.search(r"fill-between y: \d+ keys \(\d+ \.\. \d+\), 0 gaps, 0 slices filled, (\d+) -> \1 voxels", text), text

    # what the program refuses
    for args, word in ((["-fill-between"], "-fill-between needs"), (["-fill-between", "w"], "-fill-between needs")):
        res = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert res.returncode == 2 and word in res.stderr, res.stdout + res.stderr
    res = subprocess.run([str(exe), str(mhd), "-fill-between", "z"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "needs -grow" in res.stderr
