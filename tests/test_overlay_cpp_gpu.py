"""examples/render_mhd.cpp -threshold LO HI -overlay-parts 6 -overlay 96 255 with -slice z 0.5 and with -iso L (the C++ Canvas of
include/sunvolumerender/canvas.hpp: ThresholdRegion, LabelRegion, OverlayRegionOnSlice, OverlayRegion) as its own process on a phantom of
three balls, against the same steps made of the Python layer and against the numpy reference (tests/overlay_ref.py, tests/label_ref.py) on
the volume svr_volume_preprocess leaves on the device."""
import re
import subprocess

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, io, scenes
from tests import label_ref as lr
from tests import overlay_ref as ov
from tests import slice_ref as sr
from tests.cpp_example import build_example
from tests.io_util import write_mhd
from tests.test_io_cpu import GUI_COLOR, GUI_OPACITY
from tests.test_io_gpu import _preprocess

pytestmark = pytest.mark.gpu
W, H = 64, 48
FILL, EDGE = 96, 255


def three_balls():
    """bool [32][36][40]: three balls that do not touch, centred on the middle slice"""
    z, y, x = np.indices((32, 36, 40))
    out = np.zeros((32, 36, 40), dtype=bool)
    for cx, cy, cz, r in ((10, 11, 16, 7), (29, 12, 15, 8), (20, 27, 17, 6)):
        out |= (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r
    return out


def test_render_mhd_overlay_matches_python_and_numpy(hip_dev, tmp_path):
    exe = build_example(tmp_path)
    balls = three_balls()
    vol = np.where(balls, 1200, -1000).astype(np.int16)
    vol[0, 0, 0] = 2000                                                       # (the window below is the balls alone, not the brightest voxel)
    spacing = (0.8, 0.8, 1.1)
    mhd = write_mhd(tmp_path / "balls.mhd", vol, spacing)
    pre = _preprocess(hip_dev, vol, spacing)
    u16 = pre["u16"]                                                          # what the loader leaves on the device (svr_volume_preprocess)
    value = int(u16[16, 11, 10])
    lo, hi = value - 100, value + 100
    iso = float(np.float32(0.5 * value / 65535.0))                              # (a float32: the program reads the same number from its text)
    labels, parts = lr.label(balls, 6)
    assert parts == 3

    common = [str(exe), str(mhd), "-size", str(W), str(H), "-threshold", str(lo), str(hi), "-overlay-parts", "6", "-overlay", str(FILL), str(EDGE)]
    runs = {"slice": ["-slice", "z", "0.5"], "iso": ["-iso", repr(iso)]}
    for name, extra in runs.items():
        res = subprocess.run(common + extra + ["-o", str(tmp_path / f"{name}.tga")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert re.search(r"overlay parts conn 6: 3 parts", res.stdout), res.stdout

    # ---- the same steps through the Python layer
    tf = io.TransferFunction(hip_dev, GUI_OPACITY, GUI_COLOR)
    canvas = host.Canvas(hip_dev, W, H)
    try:
        canvas.SetTransferFunction(tf.Upload(), tf.maxOpacity)
        canvas.LoadVolumeFile(str(mhd))
        window = hip_dev.region_threshold(u16, lo, hi)
        assert np.array_equal(window, balls)
        dev_labels, count = hip_dev.region_label(window, 6)
        assert count == 3 and np.array_equal(dev_labels, labels)
        style = hip_dev.overlay_style(fill_alpha=FILL, edge_alpha=EDGE)
        pal = hip_dev.overlay_palette_default()
        # the numpy reference works on the volume PODs the canvas holds
        sc = scenes.Scene(name="balls", vox=u16, spacing=tuple(float(np.float32(s)) for s in spacing), max_magnitude=pre["maxMagnitude"],
                          tf_rgba=tf.compositeTable, max_opacity=tf.maxOpacity, width=W, height=H)
        R = sr.Reference(sc)
        assert bytes(R.vol.bbox) == bytes(canvas.deviceVolume.bbox)

        p = canvas.slice_params_axis(2, 0.5)
        canvas.paint_slice(p, sync=True)
        base = canvas.read_img()
        canvas.paint_slice_overlay(p, labels=dev_labels, style=style, sync=True)
        img = canvas.read_img()
        ids = ov.slice_ids(R, p, W, H, labels)[0]
        assert len(np.unique(ids)) == 4 and ov.edges(ids).any()                                       # the slice cuts the three balls
        assert np.array_equal(img, ov.blend(base, ids, pal, FILL, EDGE)) and not np.array_equal(img, base)
        assert (tmp_path / "slice.tga").read_bytes() == io.tga_encode(hip_dev, img)

        canvas.paint_projection(abi.PROJ_ISO, iso=iso, sync=True)
        base = canvas.read_img()
        hits = canvas.hit_map(abi.HIT_ISO, iso=iso)
        canvas.paint_overlay(labels=dev_labels, style=style, mode=abi.HIT_ISO, iso=iso)
        img = canvas.read_img()
        ids = ov.hit_ids(R.vol, labels, hits)
        assert len(np.unique(ids)) == 4 and (hits["status"] != abi.HIT_STATUS_FOUND).any()            # the three balls are in view
        assert np.array_equal(img, ov.blend(base, ids, pal, FILL, EDGE)) and not np.array_equal(img, base)
        assert (tmp_path / "iso.tga").read_bytes() == io.tga_encode(hip_dev, img)
    finally:
        canvas.close()
        tf.close()
