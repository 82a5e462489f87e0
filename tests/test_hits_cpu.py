"""svr_render_hits / svr_pick / svr_slice_params_through without a GPU: the ABI of the new structs, the host helper, and properties of
the test-side reference (tests/hit_ref.py) -- its consistency with the projection reference and the non-vacuity of the levels the GPU
tests use."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import hit_ref as hr
from tests import projection_ref as pr

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
f32 = np.float32

# the levels of tests/test_hits_gpu.py on tiny_head
ALPHAS = (0.0, 0.5, 0.95)
ISOS = (0.15, 0.5)


# ---------------------------------------------------------------- ABI
def _struct_fields(name):
    m = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", HEADER, flags=re.S)
    assert m, f"{name} is not declared in include/svr_abi.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float, "svr_vec3": abi.vec3}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), ctype[typ]) for n in names.split(",")]
    return fields


def test_struct_layouts_match_header():
    for name, cls, size in (("svr_hit", abi.Hit, 40), ("svr_hit_params", abi.HitParams, 12)):
        fields = _struct_fields(name)
        assert [(n, t) for n, t in cls._fields_] == fields
        off = 0
        for n, t in fields:                  # 4-byte members only: no padding
            assert getattr(cls, n).offset == off, (name, n)
            off += C.sizeof(t)
        assert C.sizeof(cls) == off == size
    assert abi.svr_hit is abi.Hit and abi.svr_hit_params is abi.HitParams
    assert [n for n, _ in abi.Hit._fields_] == ["status", "sample", "t", "value", "position", "normal"]
    assert host.HIT_DTYPE == hr.HIT_DTYPE and hr.HIT_DTYPE.itemsize == 40
    assert [hr.HIT_DTYPE.fields[n][1] for n, _ in abi.Hit._fields_] == [getattr(abi.Hit, n).offset for n, _ in abi.Hit._fields_]


def test_constants_match_header():
    def define(name):
        m = re.search(rf"#define\s+{name}\s+(\d+)u?\b", HEADER)
        assert m, name
        return int(m.group(1))

    assert (abi.HIT_OPACITY, abi.HIT_ISO, abi.HIT_MAX) == (define("SVR_HIT_OPACITY"), define("SVR_HIT_ISO"), define("SVR_HIT_MAX")) == (1, 2, 3)
    assert (abi.HIT_STATUS_MISS, abi.HIT_STATUS_NONE, abi.HIT_STATUS_FOUND) == \
        (define("SVR_HIT_STATUS_MISS"), define("SVR_HIT_STATUS_NONE"), define("SVR_HIT_STATUS_FOUND")) == (0, 1, 2)
    assert abi.PICK_MAX == define("SVR_PICK_MAX") == 4096
    assert (hr.OPACITY, hr.ISO, hr.MAX) == (abi.HIT_OPACITY, abi.HIT_ISO, abi.HIT_MAX)
    assert (hr.MISS, hr.NONE, hr.FOUND) == (abi.HIT_STATUS_MISS, abi.HIT_STATUS_NONE, abi.HIT_STATUS_FOUND)


def test_prototypes_and_defaults():
    for name in ("svr_hit_params_default", "svr_render_hits", "svr_pick", "svr_slice_params_through"):
        assert name in abi.PROTOTYPES, name
    res, args = abi.PROTOTYPES["svr_render_hits"]
    assert res is C.c_int and len(args) == 6 and args[4] is C.c_float
    res, args = abi.PROTOTYPES["svr_pick"]
    assert res is C.c_int and len(args) == 8 and args[2] is C.c_uint32 and args[6] is C.c_float
    lib = abi.load()
    lib.svr_set_error_mode(0)
    p = abi.HitParams(-1, 9.0, 9.0)
    assert lib.svr_hit_params_default(C.byref(p)) == 0                 # plain host code: no GPU needed
    assert p.as_dict() == {"mode": abi.HIT_OPACITY, "alpha": 0.5, "iso": 0.5}
    assert lib.svr_hit_params_default(None) != 0
    lib.svr_clear_error()


# ---------------------------------------------------------------- svr_slice_params_through
def _volume(clip=((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0))):
    v = host.create_device_volume(0, (40, 56, 48), (1.0, 0.8, 1.3), 1.0)
    v.x_clip, v.y_clip, v.z_clip = abi.vec2(*clip[0]), abi.vec2(*clip[1]), abi.vec2(*clip[2])
    return v


def _box(v):
    e0 = [f32(a) * -f32(c.x) for a, c in zip(v.bbox.vmin.tuple(), (v.x_clip, v.y_clip, v.z_clip))]
    e1 = [f32(a) * f32(c.y) for a, c in zip(v.bbox.vmax.tuple(), (v.x_clip, v.y_clip, v.z_clip))]
    return [min(a, b) for a, b in zip(e0, e1)], [max(a, b) for a, b in zip(e0, e1)]


@pytest.mark.parametrize("clip", [((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), ((-0.5, 0.6), (-1.0, 1.0), (-0.7, 0.4))])
def test_slice_through_equals_axis_apart_from_one_centre_component(clip):
    lib = abi.load()
    v = _volume(clip)
    lo, hi = _box(v)
    for axis in range(3):
        for w, h in ((64, 48), (33, 70)):
            # an arbitrary float inside the box, and both faces
            inner = f32(lo[axis]) + f32(0.37) * (f32(hi[axis]) - f32(lo[axis]))
            for c in (inner, lo[axis], hi[axis]):
                point = [123.5, -7.25, 1e6]                       # the other two components are not looked at (finite is enough)
                point[axis] = float(c)
                got = host.slice_params_through(lib, v, axis, point, w, h).as_dict()
                ref = host.slice_params_axis(lib, v, axis, 0.25, w, h).as_dict()
                centre = list(ref["center"])
                centre[axis] = float(f32(c))
                ref["center"] = tuple(centre)
                assert got == ref, (axis, w, h, c)
                assert np.array([got["center"][axis]], dtype=np.float32).view(np.uint32)[0] == np.array([c], dtype=np.float32).view(np.uint32)[0]


def test_slice_through_refusals():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    v = _volume()
    lo, hi = _box(v)
    P, mid = abi.SliceParams, abi.vec3(0.0, 0.0, 0.0)
    sentinel = P()
    sentinel.step = 77.0

    def call(p=True, vol=v, axis=0, point=mid, w=64, h=48):
        out = P.from_buffer_copy(sentinel)
        rc = lib.svr_slice_params_through(C.byref(out) if p else None, C.byref(vol) if vol is not None else None, axis,
                                          C.byref(point) if point is not None else None, w, h)
        lib.svr_clear_error()
        assert rc == 0 or out.step == 77.0, "a refused call wrote the parameters"
        return rc

    assert call() == 0
    flat = _volume(((-1.0, 1.0), (0.0, 0.0), (-1.0, 1.0)))          # the clipped box has no extent along y
    nan, inf = float("nan"), float("inf")
    eps_out = float(np.nextafter(f32(hi[0]), f32(np.inf)))
    refused = {
        "null params": dict(p=False), "null volume": dict(vol=None), "null point": dict(point=None),
        "axis -1": dict(axis=-1), "axis 3": dict(axis=3), "w 0": dict(w=0), "h 0": dict(h=0), "no extent": dict(vol=flat),
        "nan point": dict(point=abi.vec3(nan, 0, 0)), "inf point": dict(point=abi.vec3(inf, 0, 0)),
        "nan in another component": dict(point=abi.vec3(0, nan, 0)),
        "outside, above": dict(point=abi.vec3(eps_out, 0, 0)), "outside, below": dict(point=abi.vec3(0, 0, float(lo[2]) - 1.0), axis=2),
    }
    for what, kw in refused.items():
        assert call(**kw) != 0, f"{what} was accepted"
    # a point on a face is inside
    assert call(point=abi.vec3(float(hi[0]), 0, 0)) == 0 and call(point=abi.vec3(0, float(lo[1]), 0), axis=1) == 0
    # outside on another axis than the plane's does not matter
    assert call(point=abi.vec3(0, 1e4, 0), axis=0) == 0


# ---------------------------------------------------------------- the reference
def test_reference_agrees_with_the_projection_reference(oracle):
    """On tiny_head the ISO hit is the point projection_ref shades (n*, hi and the value fetched there), and the MAX hit's value is its
    MIP value."""
    sc = scenes.make_scene("tiny_head")
    H = hr.reference("tiny_head", lambda: sc)
    R, step = H.R, sc.step_size()
    rays = R.rays(step)
    for iso in ISOS:
        m, c = H.hit_map(hr.ISO, step, iso=iso)
        _, rc, ns = R.image(pr.ISO, step, iso=iso)
        assert c == rc, "the counts of the ISO map are the ISO projection's"
        assert np.array_equal(m["status"] == hr.MISS, ns == -2) and np.array_equal(m["status"] == hr.NONE, ns == -1)
        found = m["status"] == hr.FOUND
        assert np.array_equal(m["sample"][found], ns[found])
        for y, x in np.argwhere(found):
            n, _, hi, I_hi = R.iso_search(rays[y][x], iso)
            rec = m[y, x]
            assert rec["t"] == hi and rec["value"] == I_hi and tuple(rec["position"]) == R.point(rays[y][x], hi)
            assert rec["value"] == R.intensity(tuple(rec["position"])) and rec["value"] >= f32(iso)
    m, c = H.hit_map(hr.MAX, step)
    _, rc, M = R.image(pr.MIP, step)
    assert c["raycast_steps"] == rc["raycast_steps"]
    found = m["status"] == hr.FOUND
    assert c["vol_taps"] == rc["vol_taps"] + 6 * int(found.sum())
    assert np.array_equal(m["value"][found], M[found]) and np.all(M[m["status"] == hr.NONE] == 0)
    for y, x in np.argwhere(found):
        r, rec = rays[y][x], m[y, x]
        n = rec["sample"]
        assert r.Is[n] == rec["value"] and np.all(r.Is[:n] < rec["value"]) and np.all(r.Is <= rec["value"]) and r.ts[n] == rec["t"]
    # members not named for a status are +0, bit for bit
    for mm in (m, H.hit_map(hr.OPACITY, step)[0]):
        w = mm.view(np.uint32).reshape(sc.height, sc.width, 10)
        assert not w[mm["status"] == hr.MISS].any() and not w[mm["status"] == hr.NONE][:, 2:].any()
        assert np.all(mm["sample"][mm["status"] == hr.NONE] > 0)
    # unit normals or none
    nrm = np.linalg.norm(m["normal"][found].astype(np.float64), axis=-1)
    assert np.all((np.abs(nrm - 1) < 1e-6) | (nrm == 0)) and (nrm > 0).any()


def test_opacity_reference_is_monotone_in_alpha(oracle):
    sc = scenes.make_scene("tiny_head")
    H = hr.reference("tiny_head", lambda: sc)
    maps = [H.hit_map(hr.OPACITY, sc.step_size(), alpha=a)[0] for a in ALPHAS]
    for lo, hi in zip(maps, maps[1:]):
        both = (lo["status"] == hr.FOUND) & (hi["status"] == hr.FOUND)
        assert np.all(lo["status"][hi["status"] == hr.FOUND] == hr.FOUND), "a higher level cannot find more"
        assert np.all(lo["sample"][both] <= hi["sample"][both]) and (lo["sample"][both] < hi["sample"][both]).any()
    # alpha 0: the first sample with any opacity
    rays = H.R.rays(sc.step_size())
    m0 = maps[0]
    for y, x in np.argwhere(m0["status"] == hr.FOUND)[::7]:
        a = H.alphas((float(f32(sc.step_size())), y, x), rays[y][x])
        n = m0[y, x]["sample"]
        assert a[n] > 0 and not any(v > 0 for v in a[:n])


def test_levels_of_the_gpu_tests_are_not_vacuous(oracle):
    """Every mode, at every level tests/test_hits_gpu.py uses on tiny_head (96 x 80), has MISS, NONE and FOUND on at least 5 % of the
    pixels each."""
    sc = scenes.make_scene("tiny_head")
    assert (sc.width, sc.height) == (96, 80)
    H = hr.reference("tiny_head", lambda: sc)
    cases = [(hr.OPACITY, a, 0.5) for a in ALPHAS] + [(hr.ISO, 0.5, i) for i in ISOS] + [(hr.MAX, 0.5, 0.5)]
    for mode, alpha, iso in cases:
        m, _ = H.hit_map(mode, sc.step_size(), alpha=alpha, iso=iso)
        for status in (hr.MISS, hr.NONE, hr.FOUND):
            share = float((m["status"] == status).sum()) / m.size
            print(f"mode {mode} alpha {alpha} iso {iso} status {status}: {share:.3f}")
            assert share >= 0.05, (mode, alpha, iso, status, share)
