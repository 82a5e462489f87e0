"""examples/render_mhd.cpp -threshold LO HI -largest 1 -keep and -grow ... -minsize N (the C++ Canvas of
include/sunvolumerender/canvas.hpp: ThresholdRegion, CountRegionParts, KeepLargestRegion, RemoveSmallRegions, ShowRegion) as its own
process, against the same steps made of the Python layer and the numpy references (tests/label_ref.py, tests/region_ref.py) on the volume
svr_volume_preprocess leaves on the device."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, io, scenes
from tests import label_ref as lr
from tests import region_ref as rr
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess
from tests.cpp_example import build_example, cpp_canvas_eye

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
MEASURED = (r"(\d+) voxels, volume ([0-9.e+-]+), mean ([0-9.]+) \+- ([0-9.]+) \(raw (\d+)\.\.(\d+)\), box (\d+) (\d+) (\d+) \.\. (\d+) (\d+) (\d+), "
            r"surface ([0-9.e+-]+)")


def check_measured(m, first, u16, region, spacing):
    """The groups of MEASURED from group `first` on against the numpy statistics of `region`."""
    g = lambda i: m.group(first + i)                                           # noqa: E731
    st = rr.stats(u16, region)
    assert int(g(0)) == st["voxels"] and (int(g(4)), int(g(5))) == (st["vmin"], st["vmax"])
    assert [int(g(i)) for i in range(6, 12)] == st["bbox_min"] + st["bbox_max"]
    want = rr.measure(u16, region, [float(np.float32(s)) for s in spacing])
    assert float(g(1)) == pytest.approx(want["volume"], rel=1e-5) and float(g(12)) == pytest.approx(want["surface_area"], rel=1e-5)
    assert float(g(2)) == pytest.approx(want["mean"], abs=0.06) and float(g(3)) == pytest.approx(want["stddev"], abs=0.06)


def test_render_mhd_threshold_largest_minsize_match_python_and_numpy(hip_dev, tmp_path):
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
        # float32 throughout
        eye = cpp_canvas_eye(canvas)
        canvas.SetCamera(host.camera_setup((0.0, 0.0, eye), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), canvas.fov, canvas.apeture, canvas.focalLength,
                                           canvas.exposure, W, H))
        hit = canvas.pick([px])[0]                                            # the default -hit mode: opacity 0.5
        assert hit["status"] == abi.HIT_STATUS_FOUND
        seed = host.region_seed_from_world(hip_dev.lib, canvas.deviceVolume, (nx, ny, nz), hit["position"])
        value = int(u16[seed[2], seed[1], seed[0]])
        lo, hi = max(0, value - 6000), min(65535, value + 6000)

        # ---- -threshold LO HI -conn 18 -largest 1 -keep: the same steps in Python, and in numpy
        window = hip_dev.region_threshold(u16, lo, hi)
        labels, k = hip_dev.region_label(window, 18)
        largest, kept = hip_dev.region_select_by_size(labels, k, largest_k=1)
        want_labels, want_k = lr.label(lr.threshold(u16, lo, hi), 18)
        want_largest, want_kept = lr.select_by_size(want_labels, want_k, 0, 1)
        assert k == want_k and np.array_equal(labels, want_labels) and kept == want_kept == 1 and np.array_equal(largest, want_largest)
        out = tmp_path / "largest.tga"
        res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-threshold", str(lo), str(hi), "-conn", "18", "-largest", "1",
                              "-keep", "-o", str(out)], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        print(res.stdout)
        m = re.search(rf"threshold window {lo}\.\.{hi} conn 18: (\d+) parts, " + MEASURED, res.stdout)
        assert m, res.stdout
        assert int(m.group(1)) == k
        check_measured(m, 2, u16, window, spacing)
        m = re.search(r"largest 1 conn 18: (\d+) of (\d+) parts kept, " + MEASURED, res.stdout)
        assert m and res.stdout.index("largest 1") > res.stdout.index("threshold window"), res.stdout
        assert (int(m.group(1)), int(m.group(2))) == (1, k)
        check_measured(m, 3, u16, largest, spacing)
        assert "cleaned (" not in res.stdout                                   # that line belongs to the steps that had it
        # the frame: the ray caster on a texture of the numpy-masked volume
        masked = np.ascontiguousarray(rr.apply(u16, want_largest, rr.KEEP, 0))
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

        # ---- -threshold ... -minsize N under the default connectivity 6
        labels6, k6 = lr.label(lr.threshold(u16, lo, hi), 6)
        sizes = np.sort(np.bincount(labels6.reshape(-1))[1:])[::-1]
        n_min = int(sizes[1]) if len(sizes) > 1 else 2                         # the second largest stays, what is smaller goes
        big, kept6 = lr.select_by_size(labels6, k6, n_min, 0)
        res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-threshold", str(lo), str(hi), "-minsize", str(n_min),
                              "-o", str(tmp_path / "m.tga")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        m = re.search(rf"minsize {n_min} conn 6: (\d+) of (\d+) parts kept, " + MEASURED, res.stdout)
        assert m, res.stdout
        assert (int(m.group(1)), int(m.group(2))) == (kept6, k6)
        check_measured(m, 3, u16, big, spacing)

        # ---- -grow ... -minsize N: one grown part; at its own size it stays, one voxel more and it goes
        grown = rr.grow(u16, [seed], lo, hi, 6)
        n = int(grown.sum())
        res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-grow", str(px[0]), str(px[1]), str(lo), str(hi), "-minsize", str(n),
                              "-o", str(tmp_path / "g.tga")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert re.search(rf"conn 6: {n} voxels", res.stdout), res.stdout       # the grow line, as before
        m = re.search(rf"minsize {n} conn 6: 1 of 1 parts kept, " + MEASURED, res.stdout)
        assert m, res.stdout
        check_measured(m, 1, u16, grown, spacing)
        res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-grow", str(px[0]), str(px[1]), str(lo), str(hi), "-minsize", str(n + 1),
                              "-o", str(tmp_path / "e.tga")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and f"minsize {n + 1} conn 6: 0 of 1 parts kept; the region is empty" in res.stdout, res.stdout + res.stderr
    finally:
        hip_dev.lib.setup_volume(C.byref(canvas.deviceVolume))
        for t in texs:
            hip_dev.lib.svr_destroy_texture(t)
        canvas.close()
        tf.close()
