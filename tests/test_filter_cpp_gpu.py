"""examples/render_mhd.cpp -median 18 1 -threshold LO HI -largest 1 (the C++ Canvas of include/sunvolumerender/canvas.hpp: MedianVolume,
then ThresholdRegion and KeepLargestRegion on the filtered copy) as its own process, against the same steps made of the Python layer and
the numpy references (tests/filter_ref.py, tests/label_ref.py) on the volume svr_volume_preprocess leaves on the device."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi
from tests import filter_ref as fr
from tests import label_ref as lr
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess
from tests.test_label_cpp_gpu import MEASURED, check_measured
from tests.cpp_example import build_example

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_render_mhd_median_then_threshold_matches_python_and_numpy(hip_dev, tmp_path):
    exe = build_example(tmp_path)
    v = fr.heads()[1][:28, :36, :43].astype(np.float64)                       # the salted head; an odd nx
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000, salt at both ends
    spacing = (0.9, 0.9, 1.5)
    mhd = write_mhd(tmp_path / "ct.mhd", vol, spacing)
    u16 = _preprocess(hip_dev, vol, spacing)["u16"]                           # what the loader leaves on the device (svr_volume_preprocess)
    lo, hi = fr.BONE

    # ---- the same steps in numpy, and in Python
    want_med = fr.rank(u16, fr.MEDIAN, 18)
    med = hip_dev.volume_median(u16, 18, 1)
    assert np.array_equal(med, want_med)
    window = hip_dev.region_threshold(med, lo, hi)
    assert np.array_equal(window, fr.window(want_med))
    labels, k = lr.label(window, 6)
    k_noisy = lr.label(fr.window(u16), 6)[1]
    assert 1 <= k < k_noisy and k_noisy > 100                                 # the filter is what makes the difference
    want_largest, kept = lr.select_by_size(labels, k, 0, 1)
    assert kept == 1
    got_labels, count = hip_dev.region_label(window, 6)
    assert count == k and np.array_equal(got_labels, labels)
    largest, got_kept = hip_dev.region_select_by_size(got_labels, count, largest_k=1)
    assert got_kept == 1 and np.array_equal(largest, want_largest)

    out = tmp_path / "median.tga"
    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", "64", "48", "-median", "18", "1", "-threshold", str(lo), str(hi), "-largest", "1",
                          "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    assert re.search(r"median element 18 x 1: [0-9.]+ ms", res.stdout), res.stdout
    m = re.search(rf"threshold window {lo}\.\.{hi} conn 6: (\d+) parts, " + MEASURED, res.stdout)
    assert m and res.stdout.index("threshold window") > res.stdout.index("median element"), res.stdout
    assert int(m.group(1)) == k
    check_measured(m, 2, want_med, window, spacing)                           # the statistics are those of the FILTERED voxels
    m = re.search(r"largest 1 conn 6: (\d+) of (\d+) parts kept, " + MEASURED, res.stdout)
    assert m, res.stdout
    assert (int(m.group(1)), int(m.group(2))) == (1, k) and int(m.group(3)) == int(want_largest.sum())
    check_measured(m, 3, want_med, want_largest, spacing)

    # without the filter the same window has the noisy count
    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", "64", "48", "-threshold", str(lo), str(hi), "-o", str(out)], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    m = re.search(rf"threshold window {lo}\.\.{hi} conn 6: (\d+) parts, ", res.stdout)
    assert m and int(m.group(1)) == k_noisy, res.stdout
