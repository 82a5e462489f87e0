"""examples/render_mhd.cpp -smooth-region median|gauss SIZE [N], -smooth-parts SIZE [N] and -density SIZE (the C++ Canvas of
include/sunvolumerender/canvas.hpp: SmoothRegion, SmoothRegionParts, ShowRegionDensity) as its own process on the 48^3 head: the mask and
the class map it saves must be those of the Python layer, which tests/test_smooth_gpu.py holds against the numpy reference, and the
picture of -density the ray caster's on a texture of the reference's density volume."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, io, scenes
from tests import smooth_ref as sm
from tests.cpp_example import build_example, cpp_canvas_eye
from tests.io_util import write_mhd
from tests.test_growcut_cpp_gpu import GAIN, SHIFT, STROKES, read_u32_map
from tests.test_io_cpu import GUI_COLOR, GUI_OPACITY
from tests.test_io_gpu import _preprocess

pytestmark = pytest.mark.gpu
f32 = np.float32


def test_render_mhd_smooth_region_and_parts_match_the_python_layer(hip_dev, tmp_path):
    dev = hip_dev
    exe = build_example(tmp_path)
    v = scenes.make_ct_head_volume(48).astype(np.float64)
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000
    spacing = (0.9, 0.9, 1.5)
    mhd = write_mhd(tmp_path / "head.mhd", vol, spacing)
    u16 = _preprocess(dev, vol, spacing)["u16"]                               # what the loader leaves on the device (svr_volume_preprocess)
    sp = [float(f32(s)) for s in spacing]                                     # the C++ Canvas takes the spacing from the volume's float32 members
    lo, hi = (int(t) for t in np.percentile(u16[u16 > 0], [40, 100]))
    window = dev.region_threshold(u16, lo, hi)

    def run(*args, save="-save-mask"):
        saved = tmp_path / "saved.mhd"
        res = subprocess.run([str(exe), str(mhd), "-size", "64", "48", *args, save, str(saved), "-o", str(tmp_path / "a.tga")],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        print(res.stdout)
        return saved, res.stdout

    # ---- the region: median of a window of edge 3 (radii 1, 1, 1 at this spacing), twice; gauss of sigma 1.2
    radii, _ = host.region_smooth_radii(sp, 3.0)
    assert radii == sm.smooth_radii(sp, 3.0)[0] == (1, 1, 1)
    for args, op, r, n in ((["median", "3"], abi.SMOOTH_MAJORITY, radii, 1), (["median", "3", "2"], abi.SMOOTH_MAJORITY, radii, 2),
                           (["gauss", "1.2", "1"], abi.SMOOTH_BINOMIAL, host.smooth_radii(sp, 1.2)[0], 1)):
        saved, text = run("-raycast", "-threshold", str(lo), str(hi), "-smooth-region", *args)
        want, changed = dev.region_smooth(window, op, r, n)
        assert changed > 0 and np.array_equal(io.mhd_read(str(saved))[0].astype(bool), want), args
        m = re.search(rf"smooth-region {args[0]} {args[1]} x {n}: (\d+) -> (\d+) voxels", text)
        assert m and [int(t) for t in m.groups()] == [int(window.sum()), int(want.sum())], text
        assert np.array_equal(want, sm.smooth(window, op, r, n)[0])

    # ---- the parts: the classes of -growcut as the program saves them (tests/test_growcut_cpp_gpu.py), then smoothed by the program
    seeds = []
    for px, cls, radius in STROKES:
        seeds += ["-seed", str(px[0]), str(px[1]), str(cls)] + ([] if radius is None else [repr(radius)])
    grow = ["-slice", "z", "0.5", *seeds, "-growcut", str(GAIN), str(SHIFT)]
    saved, _ = run(*grow, save="-save-parts")
    classes = read_u32_map(saved, u16.shape)
    assert sorted(np.unique(classes).tolist()) == [1, 2, 3]
    saved, text = run(*grow, "-smooth-parts", "3", "2", save="-save-parts")
    want, changed = dev.region_label_smooth(classes, 3, radii, 2)
    assert changed > 0 and np.array_equal(read_u32_map(saved, u16.shape), want)
    assert f"smooth-parts 3 x 2 (the classes of -growcut): {changed} voxels changed their part" in text and "save-parts: the classes of -growcut" in text
    assert np.array_equal(want, sm.label_smooth(classes, 3, radii, 2)[0])

    # ---- the density: the ray caster on a texture of floor(65535 count / N) of the window (Canvas::ShowRegionDensity)
    saved, text = run("-raycast", "-threshold", str(lo), str(hi), "-density", "3")
    density = (sm.box_count(window, radii).astype(np.uint32) * 65535 // sm.box_size(radii)).astype(np.uint16)
    assert np.array_equal(dev.region_box_count(window, radii, density=True), density) and density.max() == 65535
    nz, ny, nx = u16.shape
    tf = io.TransferFunction(dev, GUI_OPACITY, GUI_COLOR)
    canvas = host.Canvas(dev, 64, 48)
    tex = 0
    try:
        canvas.SetTransferFunction(tf.Upload(), tf.maxOpacity)
        canvas.LoadVolumeFile(str(mhd))
        canvas.SetCamera(host.camera_setup((0.0, 0.0, cpp_canvas_eye(canvas)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), canvas.fov, canvas.apeture,
                                           canvas.focalLength, canvas.exposure, 64, 48))
        tex = dev.lib.svr_create_volume_texture(np.ascontiguousarray(density).ctypes.data_as(C.c_void_p), nx, ny, nz, 0, abi.LAYOUT_AUTO)
        dev.check()
        volume = abi.cudaVolume.from_buffer_copy(canvas.deviceVolume)
        volume.tex = tex
        dev.lib.setup_volume(C.byref(volume))                                 # Canvas::ShowVoxels' protocol: the shown volume is the scene's
        dev.check()
        dev.lib.render_raycasting(C.c_void_p(canvas.img), C.byref(volume), C.byref(canvas.transferFunction), C.byref(canvas.camera), C.c_float(canvas.stepSize))
        dev.check()
        dev.synchronize()
        assert (tmp_path / "a.tga").read_bytes() == io.tga_encode(dev, canvas.read_img())
    finally:
        dev.lib.setup_volume(C.byref(canvas.deviceVolume))
        if tex:
            dev.lib.svr_destroy_texture(tex)
        canvas.close()
        tf.close()

    # ---- what the program refuses
    for args, word in ((["-smooth-region", "mean", "3"], "-smooth-region needs"), (["-smooth-region", "median"], "-smooth-region needs"),
                       (["-smooth-region", "median", "3", "17"], "N must lie"), (["-smooth-parts", "-1"], "-smooth-parts needs"),
                       (["-density"], "-density needs")):
        res = subprocess.run([str(exe), str(mhd), "-threshold", str(lo), str(hi), *args], capture_output=True, text=True, timeout=120)
        assert res.returncode == 2 and word in res.stderr, res.stdout + res.stderr
    res = subprocess.run([str(exe), str(mhd), "-smooth-region", "median", "3"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "need -grow" in res.stderr
