"""examples/render_mhd.cpp -threshold LO HI -ball-open L -thickness -keep (the C++ Canvas of include/sunvolumerender/canvas.hpp:
ThresholdRegion, BallMorphRegion, RegionThickness, ShowRegion) as its own process, against the same steps made of the Python layer and the
numpy references (tests/distance_ref.py, tests/region_ref.py) on the volume svr_volume_preprocess leaves on the device."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, io, scenes
from tests import distance_ref as dr
from tests import region_ref as rr
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess
from tests.test_label_cpp_gpu import MEASURED, check_measured
from tests.cpp_example import build_example, cpp_canvas_eye

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


def test_render_mhd_ball_open_and_thickness_match_python_and_numpy(hip_dev, tmp_path):
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
    length = 1.5                                                              # in the spacing's units

    tf = io.TransferFunction(hip_dev, GUI_OPACITY, GUI_COLOR)
    canvas = host.Canvas(hip_dev, W, H)
    texs = []
    try:
        canvas.SetTransferFunction(tf.Upload(), tf.maxOpacity)
        canvas.LoadVolumeFile(str(mhd))
        # the C++ Canvas's camera: its eye distance is rounded once from double (see tests/test_region_cpp_gpu.py), the Python Canvas's is
        # float32 throughout
        eye = cpp_canvas_eye(canvas)
        canvas.SetCamera(host.camera_setup((0.0, 0.0, eye), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), canvas.fov, canvas.apeture, canvas.focalLength,
                                           canvas.exposure, W, H))
        hit = canvas.pick([px])[0]                                            # a window around what the centre pixel shows
        assert hit["status"] == abi.HIT_STATUS_FOUND
        seed = host.region_seed_from_world(hip_dev.lib, canvas.deviceVolume, (nx, ny, nz), hit["position"])
        value = int(u16[seed[2], seed[1], seed[0]])
        lo, hi = max(0, value - 6000), min(65535, value + 6000)

        # ---- the same steps in Python, and in numpy.  The C++ Canvas takes the spacing from the float32 members of the volume
        sp = [float(f32(s)) for s in spacing]
        w, unit = host.distance_weights(sp, u16.shape)
        assert (w, unit) == dr.weights(sp, u16.shape)[:2]
        r2 = int(math.floor((length / unit) ** 2))
        window = hip_dev.region_threshold(u16, lo, hi)
        opened = hip_dev.region_ball(window, abi.MORPH_OPEN, r2, weights=w)
        want = dr.ball(window, dr.OPEN, r2, w)
        assert np.array_equal(opened, want) and 0 < want.sum() < window.sum()
        dmap = hip_dev.region_distance(opened, weights=w, target=abi.DIST_TO_UNSET)
        assert np.array_equal(dmap, dr.distance_map(want, w, dr.TO_UNSET))
        max_d2, first, status = hip_dev.region_distance_max(dmap, opened)
        assert (max_d2, first, status) == dr.dmax(dmap, want) and status == rr.OK and max_d2 > 0

        out = tmp_path / "opened.tga"
        res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-threshold", str(lo), str(hi), "-ball-open", str(length), "-thickness",
                              "-keep", "-o", str(out)], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        print(res.stdout)
        m = re.search(rf"threshold window {lo}\.\.{hi} conn 6: (\d+) parts, " + MEASURED, res.stdout)
        assert m, res.stdout
        check_measured(m, 2, u16, window, spacing)
        m = re.search(rf"ball-open 1\.5 \(unit ([0-9.e+-]+), weights (\d+) (\d+) (\d+)\): " + MEASURED, res.stdout)
        assert m and res.stdout.index("ball-open") > res.stdout.index("threshold window"), res.stdout
        assert float(m.group(1)) == pytest.approx(unit, rel=1e-5) and tuple(int(m.group(i)) for i in (2, 3, 4)) == w
        check_measured(m, 5, u16, want, spacing)
        assert "cleaned (" not in res.stdout                                   # that line belongs to the steps that had it
        m = re.search(r"largest inscribed ball: radius ([0-9.e+-]+) at voxel (\d+) (\d+) (\d+)", res.stdout)
        assert m and res.stdout.index("largest inscribed ball") > res.stdout.index("ball-open"), res.stdout
        assert float(m.group(1)) == pytest.approx(math.sqrt(max_d2) * unit, rel=1e-5)
        assert [int(m.group(i)) for i in (2, 3, 4)] == [first % nx, first // nx % ny, first // nx // ny]
        # the frame: the ray caster on a texture of the numpy-masked volume
        masked = np.ascontiguousarray(rr.apply(u16, want, rr.KEEP, 0))
        tex = hip_dev.lib.svr_create_volume_texture(masked.ctypes.data_as(C.c_void_p), nx, ny, nz, 0, abi.LAYOUT_AUTO)
        hip_dev.check()
        texs.append(tex)
        volume = abi.cudaVolume.from_buffer_copy(canvas.deviceVolume)
        volume.tex = tex
        hip_dev.lib.setup_volume(C.byref(volume))                            # Canvas::ShowRegion's protocol: the shown volume is the scene's
        hip_dev.check()
        hip_dev.lib.render_raycasting(C.c_void_p(canvas.img), C.byref(volume), C.byref(canvas.transferFunction), C.byref(canvas.camera),
                                      C.c_float(canvas.stepSize))
        hip_dev.check()
        hip_dev.synchronize()
        assert out.read_bytes() == io.tga_encode(hip_dev, canvas.read_img())
    finally:
        hip_dev.lib.setup_volume(C.byref(canvas.deviceVolume))
        for t in texs:
            hip_dev.lib.svr_destroy_texture(t)
        canvas.close()
        tf.close()
