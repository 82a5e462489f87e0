"""examples/render_mhd.cpp -threshold LO HI -largest 1 -mesh out.ply -relax 2 and -mesh-iso RAW out.stl (the C++ Canvas of
include/sunvolumerender/canvas.hpp: ExtractRegionSurface, ExtractIsoSurface, SaveSurface, SurfaceMeasure) as its own process: the files
must parse and equal the meshes the Python layer makes of the same steps on the volume svr_volume_preprocess leaves on the device, and
the printed volume and area must match mesh_measure to the printed precision."""
import re
import subprocess

import numpy as np
import pytest

from sunvolumerender_amd import abi, io, scenes
from tests import mesh_ref as mr
from tests.cpp_example import build_example
from tests.io_util import write_mhd
from tests.test_io_gpu import _preprocess
from tests.test_mesh_cpu import read_ply, read_stl

pytestmark = pytest.mark.gpu
MESH_LINE = r"mesh: (\d+) vertices, (\d+) triangles, volume ([0-9.e+-]+) mm\^3, area ([0-9.e+-]+) mm\^2"


def test_render_mhd_mesh_exports_match_python(hip_dev, tmp_path):
    exe = build_example(tmp_path)
    v = scenes.make_ct_head_volume(48)[:28, :36, :44].astype(np.float64)
    vol = ((v / 65535.0) * 3000.0 - 1000.0).astype(np.int16)                 # air -1000 .. bone 2000
    spacing = (0.9, 0.9, 1.5)
    mhd = write_mhd(tmp_path / "ct.mhd", vol, spacing)
    u16 = _preprocess(hip_dev, vol, spacing)["u16"]                           # what the loader leaves on the device (svr_volume_preprocess)
    lo, hi = int(np.percentile(u16, 70)), 65535
    raw = int(np.percentile(u16, 85))
    assert 0 < lo < raw < int(u16.max())

    ply, stl = tmp_path / "region.ply", tmp_path / "iso.stl"
    res = subprocess.run([str(exe), str(mhd), "-raycast", "-size", "64", "48", "-threshold", str(lo), str(hi), "-largest", "1", "-mesh", str(ply),
                          "-relax", "2", "-mesh-iso", str(raw), str(stl), "-o", str(tmp_path / "f.tga")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    lines = re.findall(MESH_LINE, res.stdout)
    assert len(lines) == 2, res.stdout                                        # the region's line first, then the isosurface's
    assert res.stdout.index("mesh:") > res.stdout.index("largest 1")          # after the clean-up and selection steps

    # the same steps in Python; the world mapping of the volume the loader describes
    reader = io.VolumeReader(hip_dev)
    reader.Read(str(mhd))
    volume = abi.cudaVolume()
    reader.CreateDeviceVolume(volume)
    reader.ClearDevice()
    sp = [float(volume.spacing.x), float(volume.spacing.y), float(volume.spacing.z)]
    window = hip_dev.region_threshold(u16, lo, hi)
    labels, k = hip_dev.region_label(window, 6)
    largest, kept = hip_dev.region_select_by_size(labels, k, largest_k=1)
    assert kept == 1
    meshes = [hip_dev.mesh_region(largest, relax=2), hip_dev.mesh_isosurface(u16, raw)]
    wants = [mr.mesh_region(largest, 2), mr.mesh(u16, raw)]
    for (V, T, info), (wV, wT, winfo), line in zip(meshes, wants, lines):
        assert info.as_dict() == winfo and np.array_equal(V, wV) and np.array_equal(T, wT) and len(V) > 1000
        assert (int(line[0]), int(line[1])) == (len(V), len(T))
        vol6, area = hip_dev.mesh_measure(V, T, [s / 256.0 for s in sp])
        assert vol6 == mr.volume6(V, T) > 0
        assert float(line[2]) == pytest.approx(vol6 / (6.0 * 256.0 ** 3) * sp[0] * sp[1] * sp[2], rel=2e-9)     # %.9g
        assert float(line[3]) == pytest.approx(area, rel=2e-9)
    (V, T, _), (iV, iT, _) = meshes
    xyz, tri = read_ply(ply)
    assert np.array_equal(xyz, hip_dev.mesh_positions(V, volume=volume)) and np.array_equal(tri, T)
    rec = read_stl(stl)
    assert len(rec) == len(iT) and np.array_equal(rec["v"], hip_dev.mesh_positions(iV, volume=volume)[iT])
    length = np.sqrt((rec["n"].astype(np.float64) ** 2).sum(axis=1))
    assert ((np.abs(length - 1.0) < 1e-6) | (length == 0.0)).all()
    # the surface lies where the renderers draw the volume: inside its box
    lo_w = np.array([volume.bbox.vmin.x, volume.bbox.vmin.y, volume.bbox.vmin.z])
    hi_w = np.array([volume.bbox.vmax.x, volume.bbox.vmax.y, volume.bbox.vmax.z])
    assert (xyz >= lo_w - sp).all() and (xyz <= hi_w + sp).all()
