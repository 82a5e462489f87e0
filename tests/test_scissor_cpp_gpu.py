"""examples/render_mhd.cpp -scissor / -scissor-slice (the C++ Canvas of include/sunvolumerender/canvas.hpp: ScissorRegion,
ScissorRegionOnSlice, PaintRegionOnSlice) as its own process: the mask it saves must be the mask of the same chain in the Python layer,
which tests/test_scissor_gpu.py holds against the numpy reference."""
import re
import subprocess

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, io, scenes
from tests import scissor_ref as sr
from tests.cpp_example import build_example, cpp_canvas_eye
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess

pytestmark = pytest.mark.gpu


def test_render_mhd_scissor_matches_python(hip_dev, tmp_path):
    from tests.test_io_cpu import GUI_COLOR, GUI_OPACITY

    exe = build_example(tmp_path)
    v = scenes.make_ct_head_volume(48)[:28, :36, :44].astype(np.float64)
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000
    spacing = (0.9, 0.9, 1.5)
    mhd = write_mhd(tmp_path / "ct.mhd", vol, spacing)
    u16 = _preprocess(hip_dev, vol, spacing)["u16"]                           # what the loader leaves on the device (svr_volume_preprocess)
    lo, hi = (int(t) for t in np.percentile(u16[u16 > 0], [40, 80]))
    W, H = 64, 48
    triangle = [(10.25, 6.5), (50.0, 12.75), (28.5, 44.0)]
    base = [str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-threshold", str(lo), str(hi)]

    tf = io.TransferFunction(hip_dev, GUI_OPACITY, GUI_COLOR)
    canvas = host.Canvas(hip_dev, W, H)
    canvas.SetTransferFunction(tf.Upload(), tf.maxOpacity)
    canvas.LoadVolumeFile(str(mhd))
    eye = cpp_canvas_eye(canvas)                                              # the C++ Canvas's camera (see tests/test_region_cpp_gpu.py)
    cam = host.camera_setup((0.0, 0.0, eye), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), canvas.fov, canvas.apeture, canvas.focalLength, canvas.exposure, W, H)
    try:
        volume = canvas.deviceVolume
        window = hip_dev.region_threshold(u16, lo, hi)

        def run(*args):
            saved = tmp_path / "m.mhd"
            res = subprocess.run(base + list(args) + ["-save-mask", str(saved), "-o", str(tmp_path / "a.tga")], capture_output=True, text=True, timeout=120)
            assert res.returncode == 0, res.stdout + res.stderr
            print(res.stdout)
            got, _ = io.mhd_read(str(saved))
            return got.astype(bool), res.stdout

        # a polygon through the camera of the picture
        got, text = run("-scissor", "inside", *[str(t) for p in triangle for t in p])
        st = hip_dev.stencil_polygon([np.array(triangle)], W, H)
        want = hip_dev.region_scissor(window, st, volume, camera=cam, op=abi.SCISSOR_ERASE_INSIDE)
        assert np.array_equal(got, want) and 0 < want.sum() < window.sum()
        assert np.array_equal(want, window & ~sr.prism(window.shape, volume, sr.stencil_image(st, W, H)[0], camera=cam))
        m = re.search(r"scissor inside, 3 vertices: (\d+) voxels", text)
        assert m and int(m.group(1)) == want.sum(), text

        # two corners are an inclusive pixel rectangle; `outside` keeps what is seen in it
        got, text = run("-scissor", "outside", "20", "10", "45", "40")
        st = hip_dev.stencil_polygon([host.stencil_rect(20, 10, 45, 40, hip_dev.lib)], W, H)
        assert sr.stencil_image(st, W, H)[0].sum() == 26 * 31
        want = hip_dev.region_scissor(window, st, volume, camera=cam, op=abi.SCISSOR_ERASE_OUTSIDE)
        assert np.array_equal(got, want) and 0 < want.sum() < window.sum()

        # on a slice picture: cut a slab, then paint it back with a smaller polygon
        got, text = run("-scissor-slice", "z", "0.5", "inside", "4.5", "12", "8", "52", "40", "-scissor-slice", "z", "0.5", "fill", "4.5", "20", "14", "40", "30")
        sl = host.slice_params_axis(hip_dev.lib, volume, 2, 0.5, W, H)
        st1 = hip_dev.stencil_polygon([host.stencil_rect(12, 8, 52, 40, hip_dev.lib)], W, H)
        st2 = hip_dev.stencil_polygon([host.stencil_rect(20, 14, 40, 30, hip_dev.lib)], W, H)
        cut = hip_dev.region_scissor(window, st1, volume, slice=sl, w=W, h=H, op=abi.SCISSOR_ERASE_INSIDE, depth=(-2.25, 2.25))
        want = hip_dev.region_scissor(cut, st2, volume, slice=sl, w=W, h=H, op=abi.SCISSOR_FILL_INSIDE, depth=(-2.25, 2.25))
        assert np.array_equal(got, want) and cut.sum() < window.sum() and want.sum() > cut.sum() and (want & ~window).any()
        assert "scissor-slice z 0.5 thickness 4.5 inside, 4 vertices" in text and "scissor-slice z 0.5 thickness 4.5 fill, 4 vertices" in text

        # what the program refuses
        for args, word in ((["-scissor", "inside", "1", "2", "3"], "-scissor needs"), (["-scissor", "fill", "1", "2", "3", "4"], "-scissor needs"),
                           (["-scissor-slice", "w", "0.5", "inside", "1", "1", "2", "3", "4"], "-scissor-slice needs"),
                           (["-scissor-slice", "z", "0.5", "inside", "-1", "1", "2", "3", "4"], "-scissor-slice needs")):
            res = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
            assert res.returncode == 2 and word in res.stderr, res.stdout + res.stderr
    finally:
        canvas.close()
        tf.close()
    res = subprocess.run([str(exe), str(mhd), "-scissor", "inside", "1", "2", "3", "4"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "need -grow" in res.stderr
