"""The surface meshes without a GPU: the known answers of the numpy reference (tests/mesh_ref.py), the properties every mesh has (closed,
oriented, positive volume; relaxation keeps the connectivity and the cells), and the host code of the library: svr_mesh_positions, the
STL and PLY writers read back with numpy, the ABI of the new symbols, and every refusal (arguments are checked before the device is
touched) with its code."""
import ctypes as C
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import mesh_ref as mr
from tests.cpp_example import build_example
from tests.test_mesh_gpu import CASES, case, reference

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
IO_HEADER = (ROOT / "include" / "svr_io.h").read_text()


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    lib.svr_clear_error()
    return lib


def two(points):
    a = np.zeros((2, 2, 2), np.uint16)
    for x, y, z in points:
        a[z, y, x] = 2
    return a


# ---------------------------------------------------------------- the reference: known answers
def test_one_inside_voxel():
    V, T, info = mr.mesh(np.full((1, 1, 1), 2, np.uint16), 1)
    assert info == {"vertices": 8, "quads": 6, "triangles": 12, "bbox_min": [213] * 3, "bbox_max": [299] * 3, "status": mr.STATUS_OK}
    assert sorted(map(tuple, V.tolist())) == sorted((x, y, z) for x in (213, 299) for y in (213, 299) for z in (213, 299))     # 256 +- 43
    assert mr.euler(V, T) == 2 and mr.closed_and_oriented(T) and mr.volume6(V, T) == 6 * 86 ** 3
    # vertices ascend with the linear cell index: x fastest
    assert V.tolist()[:3] == [[213, 213, 213], [299, 213, 213], [213, 299, 213]]


def test_constant_volume_at_its_own_level():
    V, T, info = mr.mesh(np.full((3, 4, 5), 7, np.uint16), 7)
    assert (info["vertices"], info["triangles"]) == (96, 188)
    assert info["bbox_min"] == [256, 256, 256] and info["bbox_max"] == [256 * 5, 256 * 4, 256 * 3]
    assert mr.volume6(V, T) == 6 * 256 ** 3 * 24 and mr.euler(V, T) == 2 and mr.closed_and_oriented(T)


def test_two_voxels_touching_along_an_edge_and_at_a_corner():
    V, T, info = mr.mesh(two([(0, 0, 0), (1, 1, 0)]), 1)
    assert (info["vertices"], info["triangles"]) == (14, 24) and mr.closed_and_oriented(T)
    counts = mr.directed_edge_counts(T)
    assert counts.max() == 2 and (counts == 2).sum() == 2                        # the shared edge, once in each direction: non-manifold, expected
    V, T, info = mr.mesh(two([(0, 0, 0), (1, 1, 1)]), 1)
    assert (info["vertices"], info["triangles"]) == (15, 24) and mr.closed_and_oriented(T) and mr.directed_edge_counts(T).max() == 1


def test_ball_and_torus_have_their_euler_numbers():
    V, T, _ = mr.mesh(mr.ball(), 20000)
    assert mr.euler(V, T) == 2 and mr.closed_and_oriented(T)
    V, T, _ = mr.mesh(mr.torus(), 20000)
    assert mr.euler(V, T) == 0 and mr.closed_and_oriented(T)


def test_first_quad_by_hand():
    """One voxel: the lowest key is the z edge from padded sample (1, 1, 0) (index 4, key 14), whose far end is inside: C(-1,-1), C(-1,0),
    C(0,0), C(0,-1) in (x, y) offsets, i.e. cells (0,0,0), (0,1,0), (1,1,0), (1,0,0) = vertices 0, 2, 3, 1; the normal points to -z, out
    of the voxel."""
    V, T, _ = mr.mesh(np.full((1, 1, 1), 2, np.uint16), 1)
    assert T[:2].tolist() == [[0, 2, 3], [0, 3, 1]]
    a, b, c = (V[i].astype(np.int64) for i in T[0])
    assert np.cross(b - a, c - a).tolist() == [0, 0, -86 * 86]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_is_closed_oriented_and_encloses_a_volume(name):
    for as_mask in (False, True):
        V, T, info = reference(name, 0, as_mask)
        assert info["status"] == mr.STATUS_OK and info["triangles"] == 2 * info["quads"] == len(T) and info["vertices"] == len(V)
        assert mr.closed_and_oriented(T) and mr.volume6(V, T) > 0
        assert V.min() >= 0 and T.max() == len(V) - 1 and len(np.unique(T)) == len(V)      # every vertex is used


@pytest.mark.parametrize("name, as_mask", [("ball", True), ("noise", False), ("noise", True)])
def test_relaxation_keeps_the_triangles_and_the_cells(name, as_mask):
    vox, level = case(name)
    field = mr.mask_field(vox >= level) if as_mask else vox
    lo = 256 * mr._cells(field, 1 if as_mask else level)
    V0, T0, _ = reference(name, 0, as_mask)
    vols = [mr.volume6(V0, T0)]
    for relax in (1, 4, 16):
        V, T, info = reference(name, relax, as_mask)
        assert np.array_equal(T, T0) and V.shape == V0.shape
        assert (V >= lo).all() and (V <= lo + 256).all()
        assert info["bbox_min"] == V.min(axis=0).tolist() and info["bbox_max"] == V.max(axis=0).tolist()
        vols.append(mr.volume6(V, T))
        assert vols[-1] > 0
    if name == "ball":
        assert vols[0] > vols[1] > vols[2] > vols[3] > 0.8 * vols[0]               # it shrinks convex shapes, by a few per cent


# ---------------------------------------------------------------- ABI
def test_symbols_constants_and_structs(lib):
    raw = C.CDLL(str(abi.library_path()))
    for n in ["svr_mesh_params_default", "svr_mesh_isosurface", "svr_mesh_region", "svr_mesh_measure", "svr_mesh_positions", "svr_mesh_last_ms"]:
        assert n in abi.PROTOTYPES and hasattr(raw, n) and re.search(rf"\b{n}\s*\(", HEADER), n
    for n in ["svr_stl_write", "svr_ply_write"]:
        assert n in abi.PROTOTYPES and hasattr(raw, n) and re.search(rf"\b{n}\s*\(", IO_HEADER), n
    m = re.search(r"#define\s+SVR_MESH_ERR_CAPACITY\s+\((-?\d+)\)", HEADER)
    assert m and int(m.group(1)) == abi.MESH_ERR_CAPACITY == -11 and abi.MESH_ERR_CAPACITY not in (abi.REGION_ERR_LABEL, abi.REGION_ERR_SWEEPS)
    m = re.search(r"#define\s+SVR_MESH_MAX_RELAX\s+(\d+)", HEADER)
    assert m and int(m.group(1)) == abi.MESH_MAX_RELAX == 64
    m = re.search(r"#define\s+SVR_MESH_MAX_DIM\s+(\d+)", HEADER)
    assert m and int(m.group(1)) == abi.MESH_MAX_DIM and 256 * (abi.MESH_MAX_DIM + 2) == 2 ** 31
    assert C.sizeof(abi.MeshParams) == 8 and C.sizeof(abi.MeshInfo) == 56
    assert [getattr(abi.MeshInfo, f).offset for f in ("vertices", "quads", "triangles", "bbox_min", "bbox_max", "status")] == [0, 8, 16, 24, 36, 48]
    p = abi.MeshParams(0, 9)
    assert lib.svr_mesh_params_default(C.byref(p)) == 0 and (p.level, p.relax) == (32768, 0)
    assert lib.svr_mesh_params_default(None) == -4
    lib.svr_clear_error()
    ms = [C.c_float(7.0) for _ in range(3)]
    assert lib.svr_mesh_last_ms(*[C.byref(t) for t in ms]) == 0 and all(t.value >= 0.0 for t in ms)
    assert lib.svr_mesh_last_ms(None, None, None) == 0
    assert "svr_mesh.hip" in (ROOT / "sunvolumerender_amd" / "_build.py").read_text()


# ---------------------------------------------------------------- refusals: all are decided before the device is touched
A, V_OUT, T_OUT = 0x10000, 0x20000, 0x30000              # "device pointers": nothing is read or written through them


def _refused(lib, name, rc, code, word):
    msg = lib.svr_last_error().decode()
    last = lib.svr_last_error_code()
    lib.svr_clear_error()
    assert rc == last == code and name in msg and word in msg, (name, rc, last, msg)


def _iso(lib, vox=A, dims=(4, 4, 4), level=100, relax=0, params=True, verts=V_OUT, tris=T_OUT, info=True):
    p, i = abi.MeshParams(level, relax), abi.MeshInfo()
    i.vertices = 77
    rc = lib.svr_mesh_isosurface(C.c_void_p(vox), *dims, 1, C.byref(p) if params else None, C.c_void_p(verts), 10, C.c_void_p(tris), 10,
                                 C.byref(i) if info else None)
    assert i.vertices == 77                                                             # nothing is written on a refusal
    return rc


def _region(lib, mask=A, dims=(4, 4, 4), level=0, relax=0, params=True, verts=V_OUT, tris=T_OUT, info=True):
    p, i = abi.MeshParams(level, relax), abi.MeshInfo()
    i.vertices = 77
    rc = lib.svr_mesh_region(C.c_void_p(mask), *dims, C.byref(p) if params else None, C.c_void_p(verts), 10, C.c_void_p(tris), 10,
                             C.byref(i) if info else None)
    assert i.vertices == 77
    return rc


COMMON_REFUSALS = [
    (dict(params=False), -4, "null"), (dict(info=False), -4, "null"),
    (dict(dims=(0, 4, 4)), -6, "dimensions"), (dict(dims=(4, -1, 4)), -6, "dimensions"), (dict(dims=(4, 4, 0)), -6, "dimensions"),
    (dict(dims=(2047, 1023, 1024)), -6, "2^31 cells"), (dict(dims=(2 ** 31 - 1, 1, 1)), -6, "2^31 cells"), (dict(dims=(8388607, 1, 1)), -6, "int32"),
    (dict(relax=65), -3, "relax"), (dict(verts=None), -3, "both"), (dict(tris=None), -3, "both"),
]


@pytest.mark.parametrize("kw, code, word", COMMON_REFUSALS + [(dict(vox=None), -4, "null"), (dict(level=0), -3, "level"), (dict(level=65536), -3, "level")])
def test_isosurface_refusals(lib, kw, code, word):
    _refused(lib, "svr_mesh_isosurface", _iso(lib, **kw), code, word)


@pytest.mark.parametrize("kw, code, word", COMMON_REFUSALS + [(dict(mask=None), -4, "null")])
def test_region_refusals(lib, kw, code, word):
    _refused(lib, "svr_mesh_region", _region(lib, **kw), code, word)


def test_the_cell_limit_is_on_cells_not_voxels(lib):
    assert 2048 * 1024 * 1024 == 2 ** 31 and 2047 * 1023 * 1023 < 2 ** 31 < 2048 * 1024 * 1024 + 1      # (n + 1) per axis
    _refused(lib, "svr_mesh_region", _region(lib, dims=(2048, 1024, 1024)), -6, "2^31 cells")          # 2^31 voxels are refused here


def _measure(lib, verts=A, nv=3, tris=T_OUT, nt=1, scale=(1.0, 1.0, 1.0), vol=True, area=True):
    v, a = C.c_int64(77), C.c_double(77.0)
    s = None if scale is None else (C.c_double * 3)(*scale)
    rc = lib.svr_mesh_measure(C.c_void_p(verts), nv, C.c_void_p(tris), nt, s, C.byref(v) if vol else None, C.byref(a) if area else None)
    assert v.value == 77 and a.value == 77.0
    return rc


@pytest.mark.parametrize("kw, code, word", [
    (dict(verts=None), -4, "null"), (dict(tris=None), -4, "null"), (dict(scale=None), -4, "null"), (dict(vol=False), -4, "null"), (dict(area=False), -4, "null"),
    (dict(scale=(1.0, 0.0, 1.0)), -3, "scale"), (dict(scale=(1.0, 1.0, -2.0)), -3, "scale"), (dict(scale=(float("inf"), 1.0, 1.0)), -3, "scale"),
    (dict(scale=(1.0, float("nan"), 1.0)), -3, "scale"), (dict(nt=2 ** 32), -6, "2^32"),
])
def test_measure_refusals(lib, kw, code, word):
    _refused(lib, "svr_mesh_measure", _measure(lib, **kw), code, word)


def test_measure_of_no_triangle_needs_no_device(lib):
    v, a = C.c_int64(77), C.c_double(77.0)
    assert lib.svr_mesh_measure(None, 0, None, 0, (C.c_double * 3)(1, 1, 1), C.byref(v), C.byref(a)) == 0 and (v.value, a.value) == (0, 0.0)


# ---------------------------------------------------------------- svr_mesh_positions
def test_positions_in_millimetres_and_in_world_coordinates(lib):
    nz, ny, nx = 3, 4, 5
    V, _, info = mr.mesh(np.full((nz, ny, nx), 7, np.uint16), 7)
    spacing = (0.7, 0.9, 1.5)
    mm = host.mesh_positions(lib, V, spacing)
    assert mm.dtype == np.float32 and mm.shape == V.shape and np.array_equal(mm, mr.positions_mm(V, spacing))
    n = np.array([nx, ny, nz], np.float64)
    s = np.array(spacing, np.float64)
    assert mm.min(axis=0) == pytest.approx(0.5 * s, rel=1e-6) and mm.max(axis=0) == pytest.approx((n - 0.5) * s, rel=1e-6)
    vol = host.create_device_volume(0, (nx, ny, nz), spacing, 1.0)
    world = host.mesh_positions(lib, V, (9.0, 9.0, 9.0), vol)                   # (the spacing argument is not looked at)
    vmin = np.array([vol.bbox.vmin.x, vol.bbox.vmin.y, vol.bbox.vmin.z], np.float64)
    vmax = np.array([vol.bbox.vmax.x, vol.bbox.vmax.y, vol.bbox.vmax.z], np.float64)
    size = vmax - vmin
    assert world.min(axis=0) == pytest.approx(vmin + 0.5 / n * size, rel=1e-6) and world.max(axis=0) == pytest.approx(vmax - 0.5 / n * size, rel=1e-6)
    # every vertex: sample x sits at texture coordinate (x + 0.5) / nx of the box
    x = V.astype(np.float64) / 256.0 - 1.0
    assert world == pytest.approx(vmin + (x + 0.5) / n * size, rel=1e-6, abs=1e-6)
    rc = lib.svr_mesh_positions(V.ctypes.data_as(C.c_void_p), len(V), None, C.byref(vol), world.ctypes.data_as(C.c_void_p))
    assert rc == 0                                                               # world mode takes a NULL spacing


def test_positions_refusals(lib):
    V = np.zeros((2, 3), np.int32)
    out = np.full((2, 3), 5.0, np.float32)
    vp, op = V.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    ok = (C.c_double * 3)(1.0, 1.0, 1.0)
    _refused(lib, "svr_mesh_positions", lib.svr_mesh_positions(None, 2, ok, None, op), -4, "null")
    _refused(lib, "svr_mesh_positions", lib.svr_mesh_positions(vp, 2, ok, None, None), -4, "null")
    _refused(lib, "svr_mesh_positions", lib.svr_mesh_positions(vp, 2, None, None, op), -4, "null")
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        _refused(lib, "svr_mesh_positions", lib.svr_mesh_positions(vp, 2, (C.c_double * 3)(*bad), None, op), -3, "spacing")
    vol = host.create_device_volume(0, (5, 4, 3), (1.0, 1.0, 1.0), 1.0)
    vol.spacing.y = 0.0
    _refused(lib, "svr_mesh_positions", lib.svr_mesh_positions(vp, 2, ok, C.byref(vol), op), -3, "spacing")
    assert (out == 5.0).all()


# ---------------------------------------------------------------- STL and PLY, read back with numpy
def read_stl(path):
    raw = Path(path).read_bytes()
    n = struct.unpack_from("<I", raw, 80)[0]
    assert len(raw) == 84 + 50 * n and not raw.startswith(b"solid")
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")]), offset=84)
    return rec


def read_ply(path):
    raw = Path(path).read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int(next(ln for ln in head if ln.startswith("element vertex")).split()[-1])
    nt = int(next(ln for ln in head if ln.startswith("element face")).split()[-1])
    assert [ln for ln in head if ln.startswith("property")] == ["property float x", "property float y", "property float z",
                                                                 "property list uchar uint vertex_indices"]
    assert len(raw) == end + 12 * nv + 13 * nt
    xyz = np.frombuffer(raw, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3)
    faces = np.frombuffer(raw, dtype=np.dtype([("k", "u1"), ("i", "<u4", (3,))]), count=nt, offset=end + 12 * nv)
    assert (faces["k"] == 3).all()
    return xyz, faces["i"]


def _write(lib, name, path, xyz, tris):
    return getattr(lib, name)(str(path).encode(), xyz.ctypes.data_as(C.c_void_p), len(xyz), tris.ctypes.data_as(C.c_void_p), len(tris))


@pytest.mark.parametrize("name", ["one", "edge-touch", "noise"])
def test_stl_and_ply_round_trip(lib, tmp_path, name):
    V, T, _ = reference(name)
    xyz = host.mesh_positions(lib, V, (0.7, 0.9, 1.5))
    T = np.ascontiguousarray(T)
    if name == "one":                                                           # a degenerate facet: its normal is 0 0 0
        T = np.concatenate([T, np.array([[0, 1, 1]], np.uint32)])
    assert _write(lib, "svr_stl_write", tmp_path / "m.stl", xyz, T) == 0
    rec = read_stl(tmp_path / "m.stl")
    assert len(rec) == len(T) and (tmp_path / "m.stl").stat().st_size == 84 + 50 * len(T)
    assert np.array_equal(rec["v"], xyz[T]) and (rec["attr"] == 0).all()
    a, b, c = (xyz[T[:, k]] for k in range(3))
    u, w = (b - a).astype(np.float64), (c - a).astype(np.float64)              # (the float32 differences the writer forms)
    want = np.cross(u, w)
    length = np.sqrt((want * want).sum(axis=1))
    got_len = np.sqrt((rec["n"].astype(np.float64) ** 2).sum(axis=1))
    assert ((np.abs(got_len - 1.0) < 1e-6) | (got_len == 0.0)).all()             # unit or zero
    if name == "one":
        assert got_len[-1] == 0.0 and (got_len[:-1] > 0.0).all()
    ok = length > 1e-2 * np.sqrt((u * u).sum(axis=1) * (w * w).sum(axis=1))      # not a sliver: float32 cancellation stays small
    assert ok.sum() > len(T) // 2 and np.allclose(rec["n"][ok], want[ok] / length[ok][:, None], atol=1e-4)
    assert _write(lib, "svr_ply_write", tmp_path / "m.ply", xyz, T) == 0
    pxyz, ptri = read_ply(tmp_path / "m.ply")
    assert np.array_equal(pxyz, xyz) and np.array_equal(ptri, T)                 # the shared vertices are kept


def test_writers_refuse_bad_arrays_and_report_io_failures(lib, tmp_path):
    V, T, _ = reference("one")
    xyz = host.mesh_positions(lib, V)
    bad = np.ascontiguousarray(T).copy()
    bad[5, 2] = len(V)
    for fn in ("svr_stl_write", "svr_ply_write"):
        path = tmp_path / ("x" + fn[4:7])
        _refused(lib, fn, _write(lib, fn, path, xyz, bad), -3, "vertex")
        assert not path.exists()                                                # refused before the file is opened
        _refused(lib, fn, getattr(lib, fn)(None, xyz.ctypes.data_as(C.c_void_p), len(xyz), T.ctypes.data_as(C.c_void_p), len(T)), -4, "null")
        _refused(lib, fn, getattr(lib, fn)(str(path).encode(), None, len(xyz), T.ctypes.data_as(C.c_void_p), len(T)), -4, "null")
        rc = _write(lib, fn, tmp_path / "no" / "such" / "dir.stl", xyz, np.ascontiguousarray(T))
        assert rc == lib.svr_last_error_code() == -20 and "unable to open" in lib.svr_last_error().decode()
        lib.svr_clear_error()
    empty = np.zeros((0, 3), np.uint32)
    assert _write(lib, "svr_stl_write", tmp_path / "e.stl", xyz[:0], empty) == 0 and (tmp_path / "e.stl").stat().st_size == 84
    assert _write(lib, "svr_ply_write", tmp_path / "e.ply", xyz[:0], empty) == 0 and read_ply(tmp_path / "e.ply")[0].shape == (0, 3)


# ---------------------------------------------------------------- examples/render_mhd.cpp: the mesh arguments
@pytest.fixture(scope="module")
def render_mhd(tmp_path_factory):
    return build_example(tmp_path_factory.mktemp("render_mhd_mesh"), strict=True)


THRESHOLD = ["-threshold", "0", "10"]


@pytest.mark.parametrize("args", [["-mesh", "a.stl"], THRESHOLD + ["-mesh"], THRESHOLD + ["-mesh", "a.obj"], THRESHOLD + ["-relax", "2"],
                                  THRESHOLD + ["-mesh", "a.ply", "-relax", "65"], THRESHOLD + ["-mesh", "a.ply", "-relax", "x"],
                                  THRESHOLD + ["-mesh", "a.ply", "-relax"], ["-mesh-iso", "0", "a.stl"], ["-mesh-iso", "65536", "a.stl"],
                                  ["-mesh-iso", "100", "a.txt"], ["-mesh-iso", "100"], ["-mesh-iso", "x", "a.stl"]])
def test_render_mhd_rejects_bad_mesh_arguments(render_mhd, tmp_path, args):
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), *args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.strip(), (res.returncode, res.stderr)


def test_render_mhd_usage_names_the_mesh_exports(render_mhd):
    err = subprocess.run([str(render_mhd)], capture_output=True, text=True, timeout=60).stderr
    for word in ("-mesh FILE.stl|.ply", "-relax N", "-mesh-iso RAW FILE.stl|.ply"):
        assert word in err, word
