"""examples/render_mhd.cpp -grow (the C++ Canvas of include/sunvolumerender/canvas.hpp: VolumeReader::KeepVoxels, Canvas::Pick,
GrowRegion, ShowRegion) as its own process, against the same loop made of the Python layer, the numpy reference of the region
(tests/region_ref.py) on the volume svr_volume_preprocess leaves on the device."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, io, scenes
from tests import region_ref as rr
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess
from tests.cpp_example import build_example, cpp_canvas_eye

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


def test_render_mhd_grow_matches_python_and_numpy(hip_dev, tmp_path):
    from tests.test_io_cpu import GUI_COLOR, GUI_OPACITY

    exe = build_example(tmp_path)
    v = scenes.make_ct_head_volume(48)[:28, :36, :44].astype(np.float64)
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000
    spacing = (0.9, 0.9, 1.5)
    mhd = write_mhd(tmp_path / "ct.mhd", vol, spacing)
    u16 = _preprocess(hip_dev, vol, spacing)["u16"]                           # what the loader leaves on the device (svr_volume_preprocess)
    nz, ny, nx = u16.shape
    W, H = 64, 48
    px = (W // 2, H // 2)

    tf = io.TransferFunction(hip_dev, GUI_OPACITY, GUI_COLOR)
    canvas = host.Canvas(hip_dev, W, H)
    texs = []
    try:
        canvas.SetTransferFunction(tf.Upload(), tf.maxOpacity)
        canvas.LoadVolumeFile(str(mhd))
        # The C++ Canvas's camera.  Its ZoomToExtent (canvas.hpp, from gui/canvas.cpp:191-197) evaluates the tangent and the division in
        # double and rounds once; the Python Canvas works in float32 throughout.  For this volume the two eye distances differ by one ulp
        # (76.0477219 against 76.0477295), which the plain picture does not show and one grazing pixel of the -keep picture does.
        eye = cpp_canvas_eye(canvas)
        canvas.SetCamera(host.camera_setup((0.0, 0.0, eye), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), canvas.fov, canvas.apeture, canvas.focalLength,
                                           canvas.exposure, W, H))
        hit = canvas.pick([px])[0]                                            # the default -hit mode: opacity 0.5
        assert hit["status"] == abi.HIT_STATUS_FOUND
        seed = host.region_seed_from_world(hip_dev.lib, canvas.deviceVolume, (nx, ny, nz), hit["position"])
        value = int(u16[seed[2], seed[1], seed[0]])
        lo, hi = max(0, value - 6000), min(65535, value + 6000)
        region = rr.grow(u16, [seed], lo, hi, 18)
        st = rr.stats(u16, region)
        assert 1 < st["voxels"] < int(rr.candidates(u16, lo, hi).sum())       # a proper component: a thresholded answer differs
        images = {}
        for flag, mode in (("-keep", rr.KEEP), ("-remove", rr.REMOVE)):
            out = tmp_path / f"grow{flag}.tga"
            res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-grow", str(px[0]), str(px[1]), str(lo), str(hi), "-conn", "18",
                                  flag, "-o", str(out)], capture_output=True, text=True, timeout=120)
            assert res.returncode == 0, res.stdout + res.stderr
            m = re.search(r"conn 18: (\d+) voxels, volume ([0-9.e+-]+), mean ([0-9.]+) \+- ([0-9.]+) \(raw (\d+)\.\.(\d+)\), box (\d+) (\d+) (\d+) \.\. (\d+) (\d+) (\d+), "
                          r"surface ([0-9.e+-]+)", res.stdout)
            assert m, res.stdout
            assert int(m.group(1)) == st["voxels"] and (int(m.group(5)), int(m.group(6))) == (st["vmin"], st["vmax"])
            assert [int(m.group(i)) for i in range(7, 13)] == st["bbox_min"] + st["bbox_max"]
            want = rr.measure(u16, region, [float(np.float32(s)) for s in spacing])
            assert float(m.group(2)) == pytest.approx(want["volume"], rel=1e-5) and float(m.group(13)) == pytest.approx(want["surface_area"], rel=1e-5)
            assert float(m.group(3)) == pytest.approx(want["mean"], abs=0.06) and float(m.group(4)) == pytest.approx(want["stddev"], abs=0.06)
            # the picture: the ray caster on a texture of the numpy-masked volume
            masked = np.ascontiguousarray(rr.apply(u16, region, mode, 0))
            tex = hip_dev.lib.svr_create_volume_texture(masked.ctypes.data_as(C.c_void_p), nx, ny, nz, 0, abi.LAYOUT_AUTO)
            hip_dev.check()
            texs.append(tex)
            volume = abi.cudaVolume.from_buffer_copy(canvas.deviceVolume)
            volume.tex = tex
            hip_dev.lib.setup_volume(C.byref(volume))                        # Canvas::ShowRegion's protocol: the shown volume is the scene's
            hip_dev.check()
            hip_dev.lib.render_raycasting(C.c_void_p(canvas.img), C.byref(volume), C.byref(canvas.transferFunction), C.byref(canvas.camera),
                                          C.c_float(canvas.stepSize))
            hip_dev.check()
            hip_dev.synchronize()
            images[flag] = canvas.read_img()
            assert out.read_bytes() == io.tga_encode(hip_dev, images[flag])
        assert not np.array_equal(images["-keep"], images["-remove"])
        # a window that leaves the picked voxel out: an empty region is reported, not an error
        res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-grow", str(px[0]), str(px[1]), "0", "0", "-o", str(tmp_path / "e.tga")],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and "the region is empty" in res.stdout, res.stdout + res.stderr
    finally:
        hip_dev.lib.setup_volume(C.byref(canvas.deviceVolume))
        for t in texs:
            hip_dev.lib.svr_destroy_texture(t)
        canvas.close()
        tf.close()
