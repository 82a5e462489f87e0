"""examples/render_mhd.cpp -seed X Y CLASS [RADIUS] (three of them) -growcut GAIN SHIFT [-keep-class C] -overlay FILL EDGE with -slice z 0.5
(the C++ Canvas of include/sunvolumerender/canvas.hpp: Pick, AddSeed, GrowFromSeeds, KeepSeedClass, OverlayRegionOnSlice, SaveRegionParts)
as its own process on the 48^3 head, against the same steps made of the Python layer -- the picks, the strokes, svr_region_growcut -- on
the volume svr_volume_preprocess leaves on the device: the class map, the class sizes and the tinted slice."""
import math
import re
import subprocess

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, io, scenes
from tests.cpp_example import build_example, cpp_canvas_eye
from tests.io_util import write_mhd
from tests.test_io_cpu import GUI_COLOR, GUI_OPACITY
from tests.test_io_gpu import _preprocess

pytestmark = pytest.mark.gpu
W, H = 64, 48
FILL, EDGE = 96, 255
GAIN, SHIFT = 1, 4
STROKES = [((32, 24), 1, None), ((29, 22), 2, 2.0), ((35, 26), 3, 0.0)]       # (pixel, class, brush radius in the spacing's units or the default): the head is some 16 pixels wide


def read_u32_map(mhd, shape):
    data = re.search(r"ElementDataFile = (\S+)", mhd.read_text()).group(1)
    return np.fromfile(mhd.parent / data, dtype=np.uint32).reshape(shape)


def test_render_mhd_growcut_matches_the_python_layer(hip_dev, tmp_path):
    exe = build_example(tmp_path)
    v = scenes.make_ct_head_volume(48).astype(np.float64)
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000
    spacing = (0.9, 0.9, 1.5)
    mhd = write_mhd(tmp_path / "head.mhd", vol, spacing)
    u16 = _preprocess(hip_dev, vol, spacing)["u16"]                           # what the loader leaves on the device (svr_volume_preprocess)
    nz, ny, nx = u16.shape
    sp = [float(np.float32(s)) for s in spacing]                              # the C++ Canvas takes the spacing from the volume's float32 members
    w, unit = host.distance_weights(sp, u16.shape)

    tf = io.TransferFunction(hip_dev, GUI_OPACITY, GUI_COLOR)
    canvas = host.Canvas(hip_dev, W, H)
    try:
        canvas.SetTransferFunction(tf.Upload(), tf.maxOpacity)
        canvas.LoadVolumeFile(str(mhd))
        eye = cpp_canvas_eye(canvas)
        canvas.SetCamera(host.camera_setup((0.0, 0.0, eye), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), canvas.fov, canvas.apeture, canvas.focalLength,
                                           canvas.exposure, W, H))
        # ---- the strokes and the classes through the Python layer
        hits = canvas.pick([px for px, _, _ in STROKES])                      # the default -hit mode: opacity 0.5
        assert (hits["status"] == abi.HIT_STATUS_FOUND).all()
        markers = np.zeros(u16.shape, dtype=np.uint32)
        args = []
        for hit, (px, cls, radius) in zip(hits, STROKES):
            x, y, z = host.region_seed_from_world(hip_dev.lib, canvas.deviceVolume, (nx, ny, nz), hit["position"])
            length = 2.0 * min(sp) if radius is None else radius
            point = np.zeros(u16.shape, dtype=bool)
            point[z, y, x] = True
            stroke = hip_dev.region_ball(point, abi.MORPH_DILATE, int(math.floor((length / unit) ** 2)), weights=w)
            assert stroke[z, y, x] and (stroke.sum() > 1) == (length > 0.0)
            markers = hip_dev.region_label_paint(markers, stroke, cls, only_unlabelled=True)
            args += ["-seed", str(px[0]), str(px[1]), str(cls)] + ([] if radius is None else [repr(radius)])
        assert sorted(np.unique(markers).tolist()) == [0, 1, 2, 3]
        _, zones, info = hip_dev.region_growcut(u16, markers, gain=GAIN, shift=SHIFT, connectivity=26, want_cost=False)
        sizes = np.bincount(zones.reshape(-1), minlength=4)
        assert sizes[0] == 0 and (sizes[1:] > 0).all() and (info.unreached, info.saturated) == (0, 0)

        style = hip_dev.overlay_style(fill_alpha=FILL, edge_alpha=EDGE)
        p = canvas.slice_params_axis(2, 0.5)
        canvas.paint_slice(p, sync=True)
        base = canvas.read_img()
        canvas.paint_slice_overlay(p, labels=zones, style=style, sync=True)
        classes_img = canvas.read_img()
        assert not np.array_equal(classes_img, base)
        canvas.paint_slice(p, sync=True)
        canvas.paint_slice_overlay(p, mask=zones == 2, style=style, sync=True)
        class2_img = canvas.read_img()
        assert not np.array_equal(class2_img, base) and not np.array_equal(class2_img, classes_img)

        # ---- the program
        common = [str(exe), str(mhd), "-size", str(W), str(H), "-slice", "z", "0.5", *args, "-growcut", str(GAIN), str(SHIFT), "-overlay", str(FILL), str(EDGE)]
        res = subprocess.run(common + ["-save-parts", str(tmp_path / "classes.mhd"), "-o", str(tmp_path / "classes.tga")], capture_output=True, text=True,
                             timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert re.search(rf"growcut gain {GAIN} shift {SHIFT}, 3 strokes: 3 classes own voxels", res.stdout), res.stdout
        assert "save-parts: the classes of -growcut" in res.stdout and "SATURATED" not in res.stdout
        got = read_u32_map(tmp_path / "classes.mhd", u16.shape)
        assert np.array_equal(np.bincount(got.reshape(-1), minlength=4), sizes) and np.array_equal(got, zones)
        assert (tmp_path / "classes.tga").read_bytes() == io.tga_encode(hip_dev, classes_img)

        res = subprocess.run(common + ["-keep-class", "2", "-o", str(tmp_path / "class2.tga")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        m = re.search(r"keep-class 2: (\d+) voxels", res.stdout)
        assert m and int(m.group(1)) == sizes[2], res.stdout
        assert (tmp_path / "class2.tga").read_bytes() == io.tga_encode(hip_dev, class2_img)
    finally:
        canvas.close()
        tf.close()
