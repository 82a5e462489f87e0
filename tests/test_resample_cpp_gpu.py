"""examples/render_mhd.cpp -resample / -save-volume / -save-mask / -save-crop (the C++ Canvas of include/sunvolumerender/canvas.hpp:
ResampleVolume, SaveVolume, SaveRegion, SaveRegionCrop) as its own process, against the same steps made of the Python layer and the numpy
references (tests/resample_ref.py, tests/label_ref.py) on the volume svr_volume_preprocess leaves on the device."""
import re
import subprocess

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from sunvolumerender_amd import io as sio
from tests import filter_ref as fr
from tests import label_ref as lr
from tests import resample_ref as rr
from tests.cpp_example import build_example
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess

pytestmark = pytest.mark.gpu

SPACING = (0.9, 0.9, 1.5)
SPACING32 = tuple(float(np.float32(s)) for s in SPACING)                     # what the loader keeps (svr_volume_info.spacing is float)
LINE = r"(\d+) x (\d+) x (\d+), spacing (\S+) (\S+) (\S+), [0-9.]+ ms"


@pytest.fixture(scope="module")
def setup(hip_dev, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("render_mhd_resample")
    exe = build_example(tmp)
    v = fr.heads()[0][:28, :36, :43].astype(np.float64)                     # an odd nx
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000
    mhd = write_mhd(tmp / "ct.mhd", vol, SPACING)
    u16 = _preprocess(hip_dev, vol, SPACING)["u16"]                           # what the loader leaves on the device
    return tmp, exe, mhd, u16


def check_line(m, shape, spacing):
    assert (int(m.group(3)), int(m.group(2)), int(m.group(1))) == tuple(shape)
    assert tuple(np.float32(m.group(4 + a)) for a in range(3)) == tuple(np.float32(s) for s in spacing)


def test_render_mhd_resample_threshold_save(hip_dev, setup):
    tmp, exe, mhd, u16 = setup
    lo, hi = fr.BONE
    # ---- the same steps in numpy, and in Python
    g, applied = host.resample_grid_spacing(u16.shape, SPACING32, 0.9)
    assert (g.as_tuples(), applied) == rr.grid_spacing(u16.shape[::-1], SPACING32, (0.9, 0.9, 0.9))
    assert g.shape[0] > u16.shape[0] and g.shape[1:] == u16.shape[1:]        # z gets finer; x and y are copies (the step rounds to 65536)
    want_vol = rr.volume_resample(u16, g.as_tuples(), rr.AUTO)
    assert np.array_equal(hip_dev.volume_resample(u16, g, abi.RESAMPLE_AUTO), want_vol)
    window = fr.window(want_vol)
    labels, k = lr.label(window, 6)
    want_largest, kept = lr.select_by_size(labels, k, 0, 1)
    assert kept == 1 and want_largest.any()

    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", "64", "48", "-resample", "0.9", "-threshold", str(lo), str(hi), "-largest", "1",
                          "-save-mask", str(tmp / "m.mhd"), "-save-volume", str(tmp / "v.mhd"), "-o", str(tmp / "a.tga")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    m = re.search(r"resample 0\.9 auto: " + LINE, res.stdout)
    assert m, res.stdout
    check_line(m, g.shape, applied)
    for what in ("save-volume", "save-mask"):
        m = re.search(what + r" -> \S+: " + LINE, res.stdout)
        assert m, res.stdout
        check_line(m, g.shape, applied)
    got_vol, sp = sio.mhd_read(str(tmp / "v.mhd"))
    assert got_vol.dtype == np.uint16 and np.array_equal(got_vol, want_vol)
    assert sp == tuple(float(np.float32(s)) for s in applied)
    got_mask, sp = sio.mhd_read(str(tmp / "m.mhd"))
    assert got_mask.dtype == np.uint8 and np.array_equal(got_mask, want_largest.astype(np.uint8))
    assert np.array_equal(hip_dev.region_threshold(got_mask.astype(np.uint16), 1, 65535), want_largest)      # the way back


def test_render_mhd_save_crop(hip_dev, setup):
    tmp, exe, mhd, u16 = setup
    lo, hi = fr.BONE
    window = fr.window(u16)
    at = np.argwhere(window)
    margin = 2
    (z0, y0, x0), (z1, y1, x1) = np.maximum(at.min(0) - margin, 0), np.minimum(at.max(0) + margin, np.array(u16.shape) - 1)
    box = ((int(x0), int(y0), int(z0)), (int(x1), int(y1), int(z1)))
    want_vol = np.ascontiguousarray(u16[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1])
    want_mask = np.ascontiguousarray(window[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1])
    assert want_vol.shape != u16.shape
    sub, g = hip_dev.volume_crop(u16, box)
    assert np.array_equal(sub, want_vol) and g.as_tuples() == rr.grid_box(u16.shape[::-1], *box)
    assert np.array_equal(hip_dev.region_resample(window, g), want_mask)

    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", "64", "48", "-threshold", str(lo), str(hi), "-save-crop", str(tmp / "cv.mha"), str(tmp / "cm.mhd"),
                          str(margin), "-o", str(tmp / "b.tga")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    m = re.search(r"save-crop -> \S+ \S+: " + LINE, res.stdout)
    assert m, res.stdout
    assert (int(m.group(3)), int(m.group(2)), int(m.group(1))) == want_vol.shape
    got_vol, sp = sio.mhd_read(str(tmp / "cv.mha"))
    assert got_vol.dtype == np.uint16 and np.array_equal(got_vol, want_vol) and sp == SPACING32
    got_mask, sp = sio.mhd_read(str(tmp / "cm.mhd"))
    assert got_mask.dtype == np.uint8 and np.array_equal(got_mask, want_mask.astype(np.uint8)) and sp == SPACING32
    # the Offset is the centre of the box's first voxel in the loaded volume's centred box
    header = (tmp / "cm.mhd").read_text()
    offset = [float(t) for t in re.search(r"Offset = (\S+) (\S+) (\S+)", header).groups()]
    for a, first in enumerate((x0, y0, z0)):
        n, s = u16.shape[2 - a], SPACING32[a]
        assert abs(offset[a] - (-0.5 * n * s + (first + 0.5) * s)) <= 1e-5 * n * s
