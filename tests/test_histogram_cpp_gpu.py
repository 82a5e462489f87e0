"""examples/render_mhd.cpp -otsu CLASSES CLASS SHIFT -largest 1 and -slice z 0.5 -auto-window PLO PHI (the C++ Canvas of
include/sunvolumerender/canvas.hpp: VolumeHistogram, OtsuRegion, AutoWindow, RegionMedian) as its own process, against the same steps made
of the Python layer and the numpy references (tests/histogram_ref.py, tests/label_ref.py) on the volume svr_volume_preprocess leaves on the
device."""
import re
import subprocess

import numpy as np
import pytest

from sunvolumerender_amd import host, io, scenes
from tests import histogram_ref as hr
from tests import label_ref as lr
from tests.cpp_example import build_example
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess
from tests.test_label_cpp_gpu import MEASURED, check_measured

pytestmark = pytest.mark.gpu
f32 = np.float32


def test_render_mhd_otsu_and_auto_window_match_python_and_numpy(hip_dev, tmp_path):
    from tests.test_io_cpu import GUI_COLOR, GUI_OPACITY

    exe = build_example(tmp_path)
    v = scenes.make_ct_head_volume(48)[:28, :36, :44].astype(np.float64)
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000
    spacing = (0.9, 0.9, 1.5)
    mhd = write_mhd(tmp_path / "ct.mhd", vol, spacing)
    u16 = _preprocess(hip_dev, vol, spacing)["u16"]                           # what the loader leaves on the device (svr_volume_preprocess)
    W, H = 64, 48
    lib = hip_dev.lib

    # ---- -otsu 3 3 8 -largest 1: the brightest of three classes, in Python and in numpy
    shift = 8
    h8 = hip_dev.volume_histogram(u16, shift=shift)
    assert np.array_equal(h8, hr.histogram(u16, shift=shift))
    t, _eta = host.histogram_otsu(h8, 3, lib)
    assert t == hr.otsu(h8, 3)[0]
    thresholds = [host.histogram_bin_range(b, shift=shift, lib=lib)[1] for b in t]
    assert thresholds == [hr.bin_range(b, shift=shift)[1] for b in t]
    lo, hi = host.histogram_bin_range(t[1] + 1, shift=shift, lib=lib)[0], 65535
    window = hip_dev.region_threshold(u16, lo, hi)
    assert int(window.sum()) == int(h8[t[1] + 1:].sum()) > 0
    labels, k = hip_dev.region_label(window, 6)
    largest, kept = hip_dev.region_select_by_size(labels, k, largest_k=1)
    want_labels, want_k = lr.label(lr.threshold(u16, lo, hi), 6)
    want_largest, _ = lr.select_by_size(want_labels, want_k, 0, 1)
    assert k == want_k and kept == 1 and np.array_equal(largest, want_largest)
    median = hr.quantile(hr.histogram(u16, window), 1, 2)
    assert host.histogram_quantile(hip_dev.volume_histogram(u16, window), 1, 2, lib) == median == int(np.percentile(u16[window], 50, method="inverted_cdf"))

    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-otsu", "3", "3", str(shift), "-largest", "1", "-o", str(tmp_path / "o.tga")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    m = re.search(r"otsu 3 classes shift 8: thresholds (\d+) (\d+); class 3 window (\d+)\.\.(\d+)", res.stdout)
    assert m, res.stdout
    assert [int(m.group(1)), int(m.group(2))] == thresholds and (int(m.group(3)), int(m.group(4))) == (lo, hi)
    m = re.search(rf"threshold window {lo}\.\.{hi} conn 6: (\d+) parts, " + MEASURED, res.stdout)
    assert m and res.stdout.index("threshold window") > res.stdout.index("otsu 3 classes"), res.stdout
    assert int(m.group(1)) == k
    check_measured(m, 2, u16, window, spacing)
    m = re.search(r"median: raw (\d+)", res.stdout)
    assert m and int(m.group(1)) == median, res.stdout
    m = re.search(r"largest 1 conn 6: (\d+) of (\d+) parts kept, " + MEASURED, res.stdout)
    assert m and res.stdout.index("largest 1") > res.stdout.index("median: raw"), res.stdout
    assert (int(m.group(1)), int(m.group(2))) == (1, k)
    check_measured(m, 3, u16, largest, spacing)

    # two classes, the darker one, at the default shift
    h = hr.histogram(u16, shift=8)
    t2 = hr.otsu(h, 2)[0][0]
    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", str(W), str(H), "-otsu", "2", "1", "-o", str(tmp_path / "o2.tga")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    m = re.search(r"otsu 2 classes shift 8: threshold (\d+); class 1 window (\d+)\.\.(\d+)", res.stdout)
    assert m and [int(g) for g in m.groups()] == [hr.bin_range(t2, shift=8)[1], 0, hr.bin_range(t2, shift=8)[1]], res.stdout
    m = re.search(r"conn 6: \d+ parts, (\d+) voxels", res.stdout)
    assert m and int(m.group(1)) == int(h[:t2 + 1].sum()), res.stdout

    # ---- -slice z 0.5 -auto-window 10 990: the quantiles as the grey window, the picture against svr_render_slice under that window
    h0 = hip_dev.volume_histogram(u16)
    assert np.array_equal(h0, hr.histogram(u16))
    raw = [hr.quantile(h0, 10, 1000), hr.quantile(h0, 990, 1000)]
    assert raw == [host.histogram_quantile(h0, 10, 1000, lib), host.histogram_quantile(h0, 990, 1000, lib)] and raw[0] < raw[1]
    assert raw == [int(np.percentile(u16, q, method="inverted_cdf")) for q in (1.0, 99.0)]
    out = tmp_path / "s.tga"
    res = subprocess.run([str(exe), str(mhd), "-size", str(W), str(H), "-slice", "z", "0.5", "-auto-window", "10", "990", "-o", str(out)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    m = re.search(r"auto-window 10 990: raw (\d+)\.\.(\d+), window ([0-9.e+-]+) ([0-9.e+-]+); ", res.stdout)
    assert m and [int(m.group(1)), int(m.group(2))] == raw, res.stdout

    tf = io.TransferFunction(hip_dev, GUI_OPACITY, GUI_COLOR)
    canvas = host.Canvas(hip_dev, W, H)
    try:
        canvas.SetTransferFunction(tf.Upload(), tf.maxOpacity)
        canvas.LoadVolumeFile(str(mhd))
        scale = f32(canvas.deviceVolume.densityScale)
        win = [float(f32(f32(r) / f32(65535.0)) * scale) for r in raw]        # raw / 65535 x densityScale, in float32 as the Canvas computes it
        assert [float(f32(float(m.group(3)))), float(f32(float(m.group(4))))] == [float(f32(w)) for w in win]
        canvas.paint_slice(canvas.slice_params_axis(2, 0.5), window=(win[0], win[1]), sync=True)
        windowed = canvas.read_img()
        assert out.read_bytes() == io.tga_encode(hip_dev, windowed)
        canvas.paint_slice(canvas.slice_params_axis(2, 0.5), sync=True)      # the default window 0 .. 1 gives another picture
        assert not np.array_equal(canvas.read_img(), windowed)
    finally:
        canvas.close()
        tf.close()
