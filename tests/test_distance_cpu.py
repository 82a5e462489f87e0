"""The distance calls without a GPU: the test-side reference (tests/distance_ref.py) against an all-pairs brute force and against
scipy.ndimage.distance_transform_edt, the ball against the unit elements of tests/morph_ref.py, svr_region_distance_weights against its
definition, the ABI of the new symbols and constants, every refusal (arguments are checked before the device is touched), the new
arguments of examples/render_mhd.cpp, and the conditions the fixtures of tests/test_distance_gpu.py have to meet, asserted on the
reference."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import distance_ref as dr
from tests import morph_ref as mr
from tests import region_ref as rr
from tests.test_region_cpu import BONE, BRAIN
from tests.cpp_example import build_example

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
SOURCE = (ROOT / "sunvolumerender_amd" / "csrc" / "svr_distance.hip").read_text()


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    lib.svr_clear_error()
    return lib


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 40), (1, 9, 1), (7, 1, 1), (4, 5, 6), (3, 3, 33), (8, 8, 9), (2, 9, 33)], ids=str)
def test_reference_against_all_pairs(shape):
    assert np.prod(shape) <= 600
    for k, density in enumerate((0.0, 0.02, 0.3, 0.9, 1.0)):
        m = dr.random_mask(shape, density, 60 + k)
        for w in dr.WEIGHTS:
            for target in dr.TARGETS:
                d2, fin = dr.distance(m, w, target)
                b2, bfin = dr.brute(m, w, target)
                assert np.array_equal(fin, bfin) and np.array_equal(d2[fin], b2[bfin]), (shape, density, w, target)
                assert fin.all() or not fin.any()
                full = dr.as_map(d2, fin)
                assert (full == dr.NONE).all() == (not dr.targets(m, target).any())


@pytest.mark.parametrize("shape", rr.EDGE_SHAPES, ids=str)
def test_reference_against_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    for s in ((1, 1, 1), (1, 2, 3), (7, 7, 15)):
        w = tuple(t * t for t in s)
        for k, density in enumerate(dr.DENSITIES):
            m = dr.random_mask(shape, density, 40 + k)
            for target in dr.TARGETS:
                t = dr.targets(m, target)
                if not t.any():
                    continue                                                             # scipy's value there is not the contract's
                # distance_transform_edt measures to the nearest zero: the targets are the zeros
                want = np.rint(ndi.distance_transform_edt(~t, sampling=(s[2], s[1], s[0])) ** 2).astype(np.int64)
                d2, fin = dr.distance(m, w, target)
                assert fin.all() and np.array_equal(d2, want), (shape, s, density, target)


def test_reference_ball_select_max_volume_by_hand():
    m = np.zeros((1, 1, 9), dtype=bool)
    m[0, 0, 2] = m[0, 0, 3] = True
    dmap = dr.distance_map(m, (4, 1, 1))
    assert dmap[0, 0].tolist() == [16, 4, 0, 0, 4, 16, 36, 64, 100]
    assert dr.distance_map(m, (4, 1, 1), dr.TO_UNSET)[0, 0].tolist() == [0, 0, 4, 4, 0, 0, 0, 0, 0]
    assert dr.select(dmap, 4, 16)[0, 0].tolist() == [True, True, False, False, True, True, False, False, False]
    assert dr.ball(m, dr.DILATE, 4, (4, 1, 1))[0, 0].tolist() == [False, True, True, True, True, False, False, False, False]
    assert dr.ball(m, dr.ERODE, 3, (4, 1, 1))[0, 0].tolist() == m[0, 0].tolist() and not dr.ball(m, dr.ERODE, 4, (4, 1, 1)).any()
    assert dr.dmax(dmap) == (100, 8, rr.OK) and dr.dmax(dmap, m) == (0, 2, rr.OK) and dr.dmax(dmap, np.zeros_like(m)) == (0, 0, rr.EMPTY)
    assert dr.to_volume(dmap, 3)[0, 0].tolist() == [12, 6, 0, 0, 6, 12, 18, 24, 30]
    assert dr.to_volume(np.array([[[2, 3, dr.NONE, dr.LIMIT]]], dtype=np.uint32), 10)[0, 0].tolist() == [14, 17, 65535, 65535]
    empty = np.zeros((2, 3, 4), dtype=bool)
    assert (dr.distance_map(empty) == dr.NONE).all() and (dr.distance_map(~empty, target=dr.TO_UNSET) == dr.NONE).all()
    assert not dr.ball(empty, dr.DILATE, dr.NONE).any() and dr.ball(~empty, dr.ERODE, dr.NONE).all()      # no target: nothing grows, nothing goes


# ---------------------------------------------------------------- the ball and the unit elements
@pytest.mark.parametrize("shape", [rr.EDGE_SHAPES[0], rr.EDGE_SHAPES[5], (6, 6, 6)], ids=str)
def test_ball_of_r2_1_2_3_is_the_unit_element(shape):
    for k, density in enumerate((0.05, 0.6)):
        m = dr.random_mask(shape, density, 21)
        for r2, element in ((1, 6), (2, 18), (3, 26)):
            assert np.array_equal(dr.ball(m, dr.DILATE, r2), mr.dilate(m, element, 1)), (shape, density, element)
            assert np.array_equal(dr.ball(m, dr.ERODE, r2), mr.erode(m, element, 1)), (shape, density, element)


def test_ball_of_r2_4_is_not_the_octahedron():
    """Element 6 applied twice is the octahedron |dx| + |dy| + |dz| <= 2 (25 voxels); the ball of r2 = 4 (33 voxels) holds it and, besides,
    the eight corner offsets (+-1, +-1, +-1) of squared length 3.  Both hold the offsets (+-1, +-1, 0) and (+-2, 0, 0)."""
    m = dr.single((7, 7, 7), (3, 3, 3))
    ball, octa = dr.ball(m, dr.DILATE, 4), mr.dilate(m, 6, 2)
    assert ball.sum() == 33 and octa.sum() == 25 and not (octa & ~ball).any()
    extra = sorted(tuple(int(t) - 3 for t in p) for p in np.argwhere(ball & ~octa))
    assert extra == sorted((a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1))
    assert ball[3, 4, 4] and octa[3, 4, 4] and ball[3, 3, 5] and octa[3, 3, 5] and not ball[3, 4, 5]


# ---------------------------------------------------------------- svr_region_distance_weights
def _weights(lib, spacing, shape, w=True, unit=True, sp=True):
    nz, ny, nx = shape
    s = (C.c_double * 3)(*spacing)
    out, u = (C.c_uint32 * 3)(7, 7, 7), C.c_double(-1.0)
    rc = lib.svr_region_distance_weights(s if sp else None, nx, ny, nz, out if w else None, C.byref(u) if unit else None)
    return rc, tuple(out), u.value


@pytest.mark.parametrize("spacing, shape, k", [
    ((1.0, 1.0, 1.0), (512, 512, 512), 4), ((0.7, 0.7, 1.5), (48, 48, 48), 4), ((0.7, 0.7, 1.5), (300, 512, 512), 4),
    ((1.0, 1.0, 10.0), (512, 512, 512), 3),                                              # falls back: 25600 * 511^2 does not fit
    ((0.5, 0.25, 3.0), (2000, 100, 100), 1), ((1.0, 1.0, 1.0), (1, 1, 65536), 0), ((3.0, 2.0, 1.0), (1, 1, 1), 4),
])
def test_distance_weights_follow_their_definition(lib, spacing, shape, k):
    want_w, want_unit, want_k = dr.weights(spacing, shape)
    assert want_k == k and dr.fits(want_w, shape)
    if k < 4:                                                                             # the next finer unit must not fit
        finer = [max(1, round((s / (min(spacing) / 2 ** (k + 1))) ** 2)) for s in spacing]
        assert not dr.fits(finer, shape)
    rc, w, unit = _weights(lib, spacing, shape)
    assert rc == 0 and w == want_w and unit == want_unit == min(spacing) / 2 ** k
    assert host.distance_weights(spacing, shape, lib) == (want_w, want_unit)
    if spacing == (1.0, 1.0, 1.0) and shape == (512, 512, 512):
        assert w == (256, 256, 256)


def test_distance_weights_refusals(lib):
    for spacing in ((1.0, 1.0, 1000.0), (1.0, 1.0, 1.0)):
        shape = (512, 512, 512) if spacing[2] > 1 else (1, 2, 65537)
        with pytest.raises(ValueError):
            dr.weights(spacing, shape)
        _refused(lib, "svr_region_distance_weights", _weights(lib, spacing, shape)[0], -3, "32 bits")
    for spacing in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        with pytest.raises(ValueError):
            dr.weights(spacing, (4, 4, 4))
        rc, w, unit = _weights(lib, spacing, (4, 4, 4))
        assert w == (7, 7, 7) and unit == -1.0                                            # nothing is written on a refusal
        _refused(lib, "svr_region_distance_weights", rc, -3, "spacing")
    for kw in (dict(sp=False), dict(w=False), dict(unit=False)):
        _refused(lib, "svr_region_distance_weights", _weights(lib, (1.0, 1.0, 1.0), (4, 4, 4), **kw)[0], -4, "null")
    _refused(lib, "svr_region_distance_weights", _weights(lib, (1.0, 1.0, 1.0), (4, 0, 4))[0], -6, "dimensions")
    _refused(lib, "svr_region_distance_weights", _weights(lib, (1.0, 1.0, 1.0), (2048, 1024, 1025))[0], -6, "2^31")
    with pytest.raises(host.SvrError):
        host.distance_weights((1.0, 1.0, 1000.0), (512, 512, 512), lib)


# ---------------------------------------------------------------- ABI
def test_symbols_and_constants(lib):
    names = ["svr_region_distance", "svr_region_distance_select", "svr_region_ball", "svr_region_distance_max", "svr_region_distance_volume",
             "svr_region_distance_weights", "svr_region_distance_last_ms", "svr_region_distance_pass_ms"]
    raw = C.CDLL(str(abi.library_path()))
    for n in names:
        assert n in abi.PROTOTYPES and hasattr(raw, n), n
        assert re.search(rf"\b{n}\s*\(", HEADER), n
    for name, value in (("SVR_DIST_NONE", abi.DIST_NONE), ("SVR_DIST_TO_SET", abi.DIST_TO_SET), ("SVR_DIST_TO_UNSET", abi.DIST_TO_UNSET)):
        m = re.search(rf"#define\s+{name}\s+(\w+)", HEADER)
        assert m and int(m.group(1).rstrip("u"), 0) == value, name
    assert (abi.DIST_NONE, abi.DIST_TO_SET, abi.DIST_TO_UNSET) == (dr.NONE, dr.TO_SET, dr.TO_UNSET) == (0xFFFFFFFF, 1, 2)
    assert (abi.MORPH_DILATE, abi.MORPH_ERODE, abi.MORPH_OPEN, abi.MORPH_CLOSE) == dr.OPS
    m = re.search(r"#define\s+SVR_DISTANCE_COLUMN_BLOCK\s+(\d+)", SOURCE)
    assert m and int(m.group(1)) == abi.DISTANCE_COLUMN_BLOCK
    assert "SVR_DISTANCE_BRUTE" in SOURCE
    for dev_method in ("region_distance", "region_distance_select", "region_ball", "region_distance_max", "region_distance_volume"):
        assert callable(getattr(host.Device, dev_method))
    ms = C.c_float(7.0)
    assert lib.svr_region_distance_last_ms(C.byref(ms)) == 0 and ms.value >= 0.0
    assert lib.svr_region_distance_last_ms(None) == -4
    lib.svr_clear_error()
    assert lib.svr_region_distance_pass_ms(None, None, None) == 0
    assert lib.svr_region_distance_pass_ms(C.byref(ms), None, None) == 0 and ms.value >= 0.0


# ---------------------------------------------------------------- refusals: all are decided before the device is touched
A, B, OUT = 0x10000, 0x20000, 0x30000                   # "device pointers": nothing is read or written through them


def _refused(lib, name, rc, code, word):
    msg = lib.svr_last_error().decode()
    last = lib.svr_last_error_code()
    lib.svr_clear_error()
    assert rc == last == code and name in msg and word in msg, (name, rc, last, msg)


def _w(weights):
    return None if weights is None else (C.c_uint32 * 3)(*weights)


DIMS = [(dict(dims=(0, 4, 4)), -6, "dimensions"), (dict(dims=(4, -1, 4)), -6, "dimensions"), (dict(dims=(4, 4, 0)), -6, "dimensions"),
        (dict(dims=(2048, 1024, 1025)), -6, "2^31"), (dict(dims=(2**16, 2**16, 1)), -6, "2^31")]
# the overflow bound, at the last admissible and the first refused weight: (nx - 1)^2 = 65535^2 leaves room for exactly one;
# 3 * 1000^2 + wz * 1000^2 <= 0xFFFFFFFE holds up to wz = 4291; and an axis of 65537 is too long for any weight
WEIGHTS = [(dict(weights=(0, 1, 1)), -3, "weight"), (dict(weights=(1, 0, 1)), -3, "weight"), (dict(weights=(1, 1, 0)), -3, "weight"),
           (dict(weights=(2, 1, 1), dims=(65536, 1, 1)), -3, "overflow"), (dict(weights=(1, 1, 1), dims=(65537, 1, 1)), -3, "overflow"),
           (dict(weights=(1, 2, 4292), dims=(1001, 1001, 1001)), -3, "overflow"), (dict(weights=(0xFFFFFFFF, 1, 1), dims=(2, 1, 1)), -3, "overflow"),
           (dict(weights=(1, 0xFFFFFFFF, 0xFFFFFFFF), dims=(4, 4, 4)), -3, "overflow")]
ADMITTED = [dict(weights=(1, 1, 1), dims=(65536, 1, 1)), dict(weights=(1, 2, 4291), dims=(1001, 1001, 1001)), dict(weights=(0xFFFFFFFE, 7, 9), dims=(2, 1, 1)),
            dict(weights=(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), dims=(1, 1, 1))]


def test_the_overflow_bound_is_the_contracts():
    for kw in ADMITTED:
        nx, ny, nz = kw["dims"]
        assert dr.fits(kw["weights"], (nz, ny, nx)), kw
    for kw, code, word in WEIGHTS:
        if word == "overflow":
            nx, ny, nz = kw["dims"]
            assert not dr.fits(kw["weights"], (nz, ny, nx)), kw
    assert 3 * 1000 ** 2 + 4291 * 1000 ** 2 <= dr.LIMIT < 3 * 1000 ** 2 + 4292 * 1000 ** 2 and 65535 ** 2 <= dr.LIMIT < 2 * 65535 ** 2


def _distance(lib, inp=A, dims=(4, 4, 4), weights=None, target=1, out=OUT):
    return lib.svr_region_distance(C.c_void_p(inp), *dims, _w(weights), target, C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [(dict(inp=None), -4, "null"), (dict(out=None), -4, "null"), (dict(target=0), -3, "target"),
                                            (dict(target=3), -3, "target")] + DIMS + WEIGHTS)
def test_distance_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_distance", _distance(lib, **kw), code, word)


def _ball(lib, inp=A, dims=(4, 4, 4), op=1, weights=None, r2=1, out=OUT):
    return lib.svr_region_ball(C.c_void_p(inp), *dims, op, _w(weights), r2, C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [(dict(inp=None), -4, "null"), (dict(out=None), -4, "null"), (dict(op=0), -3, "op"), (dict(op=5), -3, "op"),
                                            (dict(out=A), -3, "overlap"), (dict(out=A + 4), -3, "overlap"), (dict(inp=OUT + 28), -3, "overlap"),
                                            (dict(out=A, r2=0), -3, "overlap")] + DIMS + WEIGHTS)
def test_ball_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_ball", _ball(lib, **kw), code, word)


def _select(lib, d2=A, dims=(4, 4, 4), lo2=0, hi2=1, out=OUT):
    return lib.svr_region_distance_select(C.c_void_p(d2), *dims, lo2, hi2, C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [(dict(d2=None), -4, "null"), (dict(out=None), -4, "null"), (dict(lo2=2), -3, "lo2"),
                                            (dict(lo2=0xFFFFFFFF, hi2=0xFFFFFFFE), -3, "lo2")] + DIMS)
def test_select_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_distance_select", _select(lib, **kw), code, word)


def _max(lib, d2=A, mask=None, dims=(4, 4, 4), outs=(True, True, True)):
    m, first, status = C.c_uint32(77), C.c_uint32(77), C.c_int32(77)
    refs = [C.byref(v) if on else None for v, on in zip((m, first, status), outs)]
    rc = lib.svr_region_distance_max(C.c_void_p(d2), C.c_void_p(mask), *dims, *refs)
    assert (m.value, first.value, status.value) == (77, 77, 77)                           # nothing is written on a refusal
    return rc


@pytest.mark.parametrize("kw, code, word", [(dict(d2=None), -4, "null"), (dict(outs=(False, True, True)), -4, "null"), (dict(outs=(True, False, True)), -4, "null"),
                                            (dict(outs=(True, True, False)), -4, "null"), (dict(d2=None, mask=B), -4, "null")] + DIMS)
def test_max_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_distance_max", _max(lib, **kw), code, word)


def _volume(lib, d2=A, dims=(4, 4, 4), scale=1, out=OUT):
    return lib.svr_region_distance_volume(C.c_void_p(d2), *dims, scale, C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [(dict(d2=None), -4, "null"), (dict(out=None), -4, "null"), (dict(scale=0), -3, "scale"),
                                            (dict(scale=65536), -3, "scale"), (dict(scale=0xFFFFFFFF), -3, "scale")] + DIMS)
def test_volume_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_distance_volume", _volume(lib, **kw), code, word)


# ---------------------------------------------------------------- conditions on the fixtures of the GPU tests
def test_gpu_cases_are_not_degenerate():
    for shape in rr.EDGE_SHAPES:
        for k, d in enumerate(dr.DENSITIES):
            m = dr.random_mask(shape, d, 40 + k)
            assert any(dr.targets(m, t).any() for t in dr.TARGETS), (shape, d)           # a target exists: a finite map
        assert dr.random_mask(shape, 0.5, 13).any() or np.prod(shape) == 1
    for name, m in dr.sparse_cases():
        assert m.any(), name
        assert (~m.any(axis=2)).any() or name == "x255", name                             # whole rows without a set voxel
    assert dr.sparse_cases()[2][1].sum() == 1 and dr.sparse_cases()[2][1][0, 0, 255]      # and one row with its only voxel at the far end
    assert (~dr.sparse_cases()[0][1].any(axis=(1, 2))).sum() == 299                       # whole slices
    for shape in dr.LONG_SHAPES:
        assert max(shape) == 2048 and all(dr.fits(w, shape) for w in dr.WEIGHTS)
        ends, every = (m for _, m in dr.long_masks(shape))
        assert ends.sum() == 2 and every.sum() == -(-np.prod(shape) // 37)
    m = dr.random_mask((64, 64, 64), 0.001, 77)
    assert 100 < m.sum() < 500


def test_gpu_shapes_cross_the_column_block():
    """One block of a column pass covers DISTANCE_COLUMN_BLOCK lanes, 32 per mask word of a row of columns (SVR_DISTANCE_COLUMN_BLOCK in
    csrc/svr_distance.hip): BLOCK_SHAPE is the smallest volume both of whose column passes need a second block."""
    block = abi.DISTANCE_COLUMN_BLOCK
    nz, ny, nx = dr.BLOCK_SHAPE
    wx = (nx + 31) // 32
    assert wx == 1 and (nz - 1) * 32 <= block < nz * 32 and (ny - 1) * 32 <= block < ny * 32
    assert any(s[0] * ((s[2] + 31) // 32) * 32 > 4 * block for s in rr.EDGE_SHAPES)      # and many blocks, with rows of several words


def test_the_maximum_is_attained_twice_in_the_tie_case():
    m = dr.tie_mask()
    dmap = dr.distance_map(m, (1, 1, 1), dr.TO_UNSET)
    at = np.flatnonzero(dmap.reshape(-1) == dmap.max())
    assert dmap.max() == dr.TIE_D2 and at.tolist() == [dr.TIE_INDEX, dr.TIE_INDEX + 5] and dr.dmax(dmap, m) == (dr.TIE_D2, dr.TIE_INDEX, rr.OK)


def test_head_masks_inscribed_radius():
    """The inscribed radius^2 of the tiny_head masks under weights (1, 1, 1), from the reference alone: the brain holds a ball of radius^2
    46.  The bone window is a shell two voxels thick: its radius^2 is 2 (scipy.ndimage.distance_transform_edt agrees), below the 4 that the
    plan for these tests assumed, so the GPU loop closes the bone mask -- which thickens it -- and measures the thickness on the brain."""
    head = scenes.make_scene("tiny_head").vox
    brain = (head >= BRAIN[0]) & (head <= BRAIN[1])
    bone = (head >= BONE[0]) & (head <= BONE[1])
    assert dr.dmax(dr.cached_map("head-brain", brain, (1, 1, 1), dr.TO_UNSET), brain)[0] == 46 >= 4
    assert dr.dmax(dr.cached_map("head-bone", bone, (1, 1, 1), dr.TO_UNSET), bone)[0] == 2


# ---------------------------------------------------------------- examples/render_mhd.cpp: the ball arguments
@pytest.fixture(scope="module")
def render_mhd(tmp_path_factory):
    exe = build_example(tmp_path_factory.mktemp("render_mhd_distance"), strict=True)
    return exe


THRESHOLD = ["-threshold", "0", "10"]


@pytest.mark.parametrize("args", [THRESHOLD + ["-ball-open"], THRESHOLD + ["-ball-open", "0"], THRESHOLD + ["-ball-close", "-2"], THRESHOLD + ["-ball-dilate", "x"],
                                  THRESHOLD + ["-ball-erode", "1.5mm"], THRESHOLD + ["-ball-erode", "inf"], THRESHOLD + ["-ball-erode", "nan"],
                                  THRESHOLD + ["-ball-shrink", "2"], ["-ball-open", "2"], ["-ball-close", "2.5"], ["-thickness"]])
def test_render_mhd_rejects_bad_ball_arguments(render_mhd, tmp_path, args):
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), *args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.strip(), (res.returncode, res.stderr)


def test_render_mhd_usage_names_the_ball_steps(render_mhd):
    err = subprocess.run([str(render_mhd)], capture_output=True, text=True, timeout=60).stderr
    for word in ("-ball-dilate L", "-ball-erode L", "-ball-open L", "-ball-close L", "-thickness"):
        assert word in err, word
