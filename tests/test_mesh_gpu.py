"""svr_mesh_isosurface / svr_mesh_region / svr_mesh_measure on the GPU against the numpy reference (tests/mesh_ref.py): vertices, triangles
and info must be EQUAL -- everything is integer -- from a host array, a device pointer and an uploaded mask; the sizing protocol; the
measures; relaxation; the chain threshold -> largest -> mesh."""
import ctypes as C
import functools

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import mesh_ref as mr

pytestmark = pytest.mark.gpu


def _two(points):
    a = np.zeros((2, 2, 2), np.uint16)
    for x, y, z in points:
        a[z, y, x] = 2
    return a


def _rng(shape, seed, hi):
    return np.random.default_rng(seed).integers(0, hi, size=shape).astype(np.uint16)


# name -> (volume, level): the smallest shapes at which the passes can go wrong
CASES = {
    "one": lambda: (np.full((1, 1, 1), 2, np.uint16), 1),
    "edge-touch": lambda: (_two([(0, 0, 0), (1, 1, 0)]), 1),
    "corner-touch": lambda: (_two([(0, 0, 0), (1, 1, 1)]), 1),
    "flat": lambda: (_rng((1, 7, 33), 3, 3), 1),
    "line": lambda: (_rng((1, 1, 70), 4, 3), 1),
    "nx31": lambda: (mr.noise((3, 4, 31), 31), 32768),
    "nx32": lambda: (mr.noise((3, 4, 32), 32), 32768),
    "nx33": lambda: (mr.noise((3, 4, 33), 33), 32768),
    "nx65": lambda: (mr.noise((3, 4, 65), 65), 32768),
    "nx62": lambda: (mr.noise((2, 3, 62), 62), 32768),                     # the padded row fills one wave exactly
    "nx63": lambda: (mr.noise((2, 3, 63), 63), 32768),                     # ... and spills one point into a second
    "noise": lambda: (mr.noise((5, 9, 37), 7), 32768),                     # every ambiguous cell configuration
    "all-inside": lambda: (np.full((3, 4, 5), 7, np.uint16), 7),           # the surface lies on the virtual border only
    "big": lambda: (mr.noise((40, 40, 70), 9), 40000),                     # more than a block of waves on every axis, no multiple of anything
    "ball": lambda: (mr.ball(), 20000),
}


@functools.lru_cache(maxsize=None)
def case(name):
    vox, level = CASES[name]()
    vox.setflags(write=False)
    return vox, level


@functools.lru_cache(maxsize=None)
def reference(name, relax=0, as_mask=False):
    vox, level = case(name)
    V, T, info = mr.mesh_region(vox >= level, relax) if as_mask else mr.mesh(vox, level, relax)
    V.setflags(write=False)
    T.setflags(write=False)
    return V, T, info


def check(got, want, what):
    V, T, info = got
    wV, wT, winfo = want
    d = info.as_dict()
    print(what, d)
    assert d == winfo, what
    assert V.dtype == np.int32 and T.dtype == np.uint32 and V.shape == wV.shape and T.shape == wT.shape, what
    assert np.array_equal(V, wV), what
    assert np.array_equal(T, wT), what


def upload(dev, arr):
    buf = dev.malloc(max(arr.nbytes, 4))
    dev.to_device(buf, arr)
    return buf


@pytest.mark.parametrize("name", sorted(CASES))
def test_isosurface_from_a_host_array_equals_the_reference(hip_dev, name):
    vox, level = case(name)
    check(hip_dev.mesh_isosurface(vox, level), reference(name), name)


@pytest.mark.parametrize("name", ["one", "nx33", "noise", "big"])
def test_isosurface_from_a_device_pointer_equals_the_reference(hip_dev, name):
    vox, level = case(name)
    buf = upload(hip_dev, vox)
    try:
        check(hip_dev.mesh_isosurface(buf, level, shape=vox.shape), reference(name), name)
    finally:
        hip_dev.free(buf)


@pytest.mark.parametrize("name", sorted(CASES))
def test_region_from_an_uploaded_mask_equals_the_reference(hip_dev, name):
    vox, level = case(name)
    check(hip_dev.mesh_region(vox >= level), reference(name, as_mask=True), name)


@pytest.mark.parametrize("name", ["nx31", "nx32", "nx33", "nx65", "flat", "line"])
def test_garbage_in_the_padding_bits_of_a_mask_is_ignored(hip_dev, name):
    vox, level = case(name)
    nz, ny, nx = vox.shape
    words = host.region_mask_pack(vox >= level).reshape(nz, ny, -1).copy()
    if nx % 32:
        words[:, :, -1] |= np.uint32((0xffffffff << (nx % 32)) & 0xffffffff)
    else:
        assert name == "nx32"                                                 # no padding bits: the word edge itself
    buf = upload(hip_dev, words)
    try:
        check(hip_dev.mesh_region(buf, shape=vox.shape), reference(name, as_mask=True), name)
    finally:
        hip_dev.free(buf)


def test_an_all_outside_volume_gives_an_empty_mesh(hip_dev):
    vox = np.zeros((3, 4, 5), np.uint16)
    want = mr.mesh(vox, 1)
    assert want[2]["status"] == mr.STATUS_EMPTY and want[2]["bbox_min"] == [256 * 7, 256 * 6, 256 * 5] and want[2]["bbox_max"] == [-1, -1, -1]
    check(hip_dev.mesh_isosurface(vox, 1), want, "empty iso")
    check(hip_dev.mesh_region(vox > 0), want, "empty mask")
    p, info = hip_dev.mesh_params(1), abi.MeshInfo()
    rc = hip_dev.lib.svr_mesh_isosurface(vox.ctypes.data_as(C.c_void_p), 5, 4, 3, 0, C.byref(p), C.c_void_p(0x1000), 0, C.c_void_p(0x2000), 0, C.byref(info))
    assert rc == 0 and info.status == abi.REGION_STATUS_EMPTY == mr.STATUS_EMPTY and info.vertices == 0      # nothing to write: capacity 0 is enough


def test_a_sample_at_the_level_is_inside_and_one_below_is_not(hip_dev):
    vox = np.zeros((3, 3, 3), np.uint16)
    vox[1, 1, 1] = 1000
    at = hip_dev.mesh_isosurface(vox, 1000)
    check(at, mr.mesh(vox, 1000), "v == level")
    assert at[2].vertices == 8 and np.array_equal(np.unique(at[0]), [512])     # q = 256: all crossing points sit on the sample itself
    vox[1, 1, 1] = 999
    below = hip_dev.mesh_isosurface(vox, 1000)
    check(below, mr.mesh(vox, 1000), "v == level - 1")
    assert below[2].vertices == 0 and below[2].status == abi.REGION_STATUS_EMPTY


@pytest.mark.parametrize("relax", [1, 4, 16])
def test_relaxation_equals_the_reference(hip_dev, relax):
    vox, level = case("ball")
    check(hip_dev.mesh_region(vox >= level, relax), reference("ball", relax, True), f"ball mask relax {relax}")
    vox, level = case("noise")
    check(hip_dev.mesh_isosurface(vox, level, relax), reference("noise", relax), f"noise relax {relax}")
    check(hip_dev.mesh_region(vox >= level, relax), reference("noise", relax, True), f"noise mask relax {relax}")


def test_sizing_protocol(hip_dev):
    vox, level = case("noise")
    wV, wT, winfo = reference("noise")
    nv, nt = len(wV), len(wT)
    nz, ny, nx = vox.shape
    lib, p = hip_dev.lib, hip_dev.mesh_params(level)
    src = vox.ctypes.data_as(C.c_void_p)
    pattern_v, pattern_t = np.full((nv + 1, 3), -12345, np.int32), np.full((nt + 1, 3), 0xabcdef01, np.uint32)
    vbuf, tbuf = upload(hip_dev, pattern_v), upload(hip_dev, pattern_t)

    def call(v, vcap, t, tcap):
        info = abi.MeshInfo()
        rc = lib.svr_mesh_isosurface(src, nx, ny, nz, 0, C.byref(p), v, vcap, t, tcap, C.byref(info))
        lib.svr_clear_error()
        return rc, info.as_dict()
    try:
        assert call(None, 0, None, 0) == (0, winfo)                           # a counting call
        assert call(None, nv, None, nt) == (0, winfo)
        for vcap, tcap in ((nv - 1, nt), (nv, nt - 1), (0, 0)):              # too small: the info, the code, and nothing written
            assert call(C.c_void_p(vbuf), vcap, C.c_void_p(tbuf), tcap) == (abi.MESH_ERR_CAPACITY, winfo) and abi.MESH_ERR_CAPACITY == -11
            assert np.array_equal(hip_dev.to_host(vbuf, pattern_v.shape, np.int32), pattern_v)
            assert np.array_equal(hip_dev.to_host(tbuf, pattern_t.shape, np.uint32), pattern_t)
        assert call(C.c_void_p(vbuf), nv, C.c_void_p(tbuf), nt) == (0, winfo)     # the exact capacity
        gV, gT = hip_dev.to_host(vbuf, pattern_v.shape, np.int32), hip_dev.to_host(tbuf, pattern_t.shape, np.uint32)
        assert np.array_equal(gV[:nv], wV) and np.array_equal(gT[:nt], wT)
        assert np.array_equal(gV[nv:], pattern_v[nv:]) and np.array_equal(gT[nt:], pattern_t[nt:])      # and nothing past the end
    finally:
        hip_dev.free(vbuf)
        hip_dev.free(tbuf)


@pytest.mark.parametrize("name, relax", [("one", 0), ("edge-touch", 0), ("all-inside", 0), ("noise", 0), ("ball", 0), ("ball", 4), ("big", 0)])
def test_measure_volume_exact_and_area_to_rounding(hip_dev, name, relax):
    V, T, _ = reference(name, relax)
    scale = (0.7 / 256, 0.9 / 256, 1.5 / 256)
    vol6, area = hip_dev.mesh_measure(V, T, scale)
    want6, want_area = mr.volume6(V, T), mr.area(V, T, scale)
    print(name, relax, vol6, want6, area, want_area)
    assert vol6 == want6 and vol6 > 0
    assert abs(area - want_area) <= 1e-9 * want_area
    if name == "all-inside":
        assert vol6 == 6 * 256 ** 3 * 24


def test_measure_refuses_an_index_out_of_range(hip_dev):
    V, T, _ = reference("one")
    bad = T.copy()
    bad[3, 1] = len(V)
    with pytest.raises(host.SvrError, match="svr_mesh_measure"):
        hip_dev.mesh_measure(V, bad)
    assert hip_dev.mesh_measure(V, T[:0]) == (0, 0.0)


def test_chain_threshold_largest_mesh(hip_dev):
    u16 = np.ascontiguousarray(scenes.make_ct_head_volume(48))
    lo, hi = 30000, 65535
    window = hip_dev.region_threshold(u16, lo, hi)
    labels, k = hip_dev.region_label(window, 6)
    largest, kept = hip_dev.region_select_by_size(labels, k, largest_k=1)
    assert kept == 1 and 1000 < largest.sum() <= window.sum()
    kept_vox = hip_dev.region_apply(u16, largest, abi.REGION_KEEP, 0)
    want = mr.mesh(np.where(kept_vox > 0, 2, 0).astype(np.uint16), 1)
    got = hip_dev.mesh_region(largest)
    check(got, want, "chain")
    assert mr.closed_and_oriented(got[1]) and mr.volume6(got[0], got[1]) > 0
    ms = hip_dev.mesh_last_ms()
    assert ms[0] > 0.0 and ms[1] > 0.0 and ms[2] == 0.0
