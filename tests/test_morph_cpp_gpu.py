"""examples/render_mhd.cpp -grow ... -detach 1 -fillholes (the C++ Canvas of include/sunvolumerender/canvas.hpp: GrowRegion, DetachRegion,
FillRegionHoles, ShowRegion) as its own process, against the same steps made of the Python layer and the numpy references
(tests/region_ref.py, tests/morph_ref.py) on the volume svr_volume_preprocess leaves on the device."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, io, scenes
from tests import morph_ref as mr
from tests import region_ref as rr
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess
from tests.cpp_example import build_example, cpp_canvas_eye

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


def test_render_mhd_detach_fillholes_matches_python_and_numpy(hip_dev, tmp_path):
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
        # the C++ Canvas's camera: its eye distance is rounded once from double (see tests/test_region_cpp_gpu.py), the Python Canvas's is
        # float32 throughout; one ulp apart for this volume, which one grazing pixel of the -keep picture shows
        eye = cpp_canvas_eye(canvas)
        canvas.SetCamera(host.camera_setup((0.0, 0.0, eye), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), canvas.fov, canvas.apeture, canvas.focalLength,
                                           canvas.exposure, W, H))
        hit = canvas.pick([px])[0]                                            # the default -hit mode: opacity 0.5
        assert hit["status"] == abi.HIT_STATUS_FOUND
        seed = host.region_seed_from_world(hip_dev.lib, canvas.deviceVolume, (nx, ny, nz), hit["position"])
        value = int(u16[seed[2], seed[1], seed[0]])
        lo, hi = max(0, value - 6000), min(65535, value + 6000)
        # the same steps in Python: grow (connectivity 18, which DetachRegion reuses), detach 6 / 1 from the seed, fill with background 6
        grown, _ = hip_dev.region_grow(u16, [seed], lo, hi, 18)
        detached, status = hip_dev.region_detach(grown, [seed], 6, 1, 18)
        cleaned = hip_dev.region_fill_holes(detached, 6)
        assert np.array_equal(grown, rr.grow(u16, [seed], lo, hi, 18))
        want_detached, want_status = mr.detach(grown, [seed], 6, 1, 18)
        assert status == want_status and np.array_equal(detached, want_detached) and np.array_equal(cleaned, mr.fill_holes(want_detached, 6))
        st = rr.stats(u16, cleaned)
        print(f"grown {int(grown.sum())}, detached {int(detached.sum())}, cleaned {st['voxels']} voxels")

        out = tmp_path / "cleaned.tga"
        res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-grow", str(px[0]), str(px[1]), str(lo), str(hi), "-conn", "18",
                              "-detach", "1", "-fillholes", "-o", str(out)], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert re.search(rf"conn 18: {int(grown.sum())} voxels", res.stdout), res.stdout          # the grow line, as before
        if st["status"] == rr.EMPTY:
            assert "cleaned (detach 1 fillholes, element 6): the region is empty" in res.stdout, res.stdout
        else:
            m = re.search(r"cleaned \(detach 1 fillholes, element 6\): (\d+) voxels, volume ([0-9.e+-]+), mean ([0-9.]+) \+- ([0-9.]+) \(raw (\d+)\.\.(\d+)\), "
                          r"box (\d+) (\d+) (\d+) \.\. (\d+) (\d+) (\d+), surface ([0-9.e+-]+)", res.stdout)
            assert m, res.stdout
            assert res.stdout.index("cleaned") > res.stdout.index("conn 18:")
            assert int(m.group(1)) == st["voxels"] and (int(m.group(5)), int(m.group(6))) == (st["vmin"], st["vmax"])
            assert [int(m.group(i)) for i in range(7, 13)] == st["bbox_min"] + st["bbox_max"]
            want = rr.measure(u16, cleaned, [float(np.float32(s)) for s in spacing])
            assert float(m.group(2)) == pytest.approx(want["volume"], rel=1e-5) and float(m.group(13)) == pytest.approx(want["surface_area"], rel=1e-5)
            assert float(m.group(3)) == pytest.approx(want["mean"], abs=0.06) and float(m.group(4)) == pytest.approx(want["stddev"], abs=0.06)
        # the frame: the ray caster on a texture of the numpy-masked volume
        masked = np.ascontiguousarray(rr.apply(u16, cleaned, rr.KEEP, 0))
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
        # every other step goes through the same calls: they run and report
        res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-grow", str(px[0]), str(px[1]), str(lo), str(hi), "-element", "26",
                              "-close", "1", "-open", "1", "-dilate", "2", "-erode", "2", "-o", str(tmp_path / "m.tga")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and "cleaned (close 1 open 1 dilate 2 erode 2, element 26):" in res.stdout, res.stdout + res.stderr
        g6 = rr.grow(u16, [seed], lo, hi, 6)
        chain = mr.morph(mr.morph(mr.morph(mr.morph(g6, mr.CLOSE, 26, 1), mr.OPEN, 26, 1), mr.DILATE, 26, 2), mr.ERODE, 26, 2)
        n = re.search(r"element 26\): (\d+) voxels", res.stdout)
        assert (int(n.group(1)) if n else 0) == int(chain.sum()), res.stdout
    finally:
        hip_dev.lib.setup_volume(C.byref(canvas.deviceVolume))
        for t in texs:
            hip_dev.lib.svr_destroy_texture(t)
        canvas.close()
        tf.close()
