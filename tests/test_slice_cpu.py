"""Slice views without a GPU: the ABI of svr_slice_params, the host-side helpers svr_slice_params_default / svr_slice_params_axis,
properties of the test-side reference (tests/slice_ref.py), and the min side of the skipping argument of csrc/svr_slice.hip checked
directly against the oracle's sampler."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import slice_ref as sr

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
f32 = np.float32


# ---------------------------------------------------------------- ABI
def test_struct_layout_matches_header():
    m = re.search(r"typedef struct svr_slice_params \{(.*?)\} svr_slice_params;", HEADER, flags=re.S)
    assert m, "svr_slice_params is not declared in include/svr_abi.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float, "svr_vec3": abi.vec3}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(n.strip(), ctype[typ]) for n in names.split(",")]
    assert [n for n, _ in fields] == ["center", "u", "v", "thickness", "step", "mode", "flags", "window_lo", "window_hi"]
    assert [(n, t) for n, t in abi.SliceParams._fields_] == fields
    off = 0
    for n, t in fields:                      # 4-byte members (svr_vec3 = three floats): no padding
        assert getattr(abi.SliceParams, n).offset == off, n
        assert C.sizeof(t) in (4, 12) and C.alignment(t) == 4
        off += C.sizeof(t)
    assert C.sizeof(abi.SliceParams) == off == 60
    assert abi.svr_slice_params is abi.SliceParams


def test_constants_match_header():
    def define(name):
        m = re.search(rf"#define\s+{name}\s+(\d+)u?\b", HEADER)
        assert m, name
        return int(m.group(1))

    assert (abi.SLAB_MIP, abi.SLAB_MINIP, abi.SLAB_MEAN) == (define("SVR_SLAB_MIP"), define("SVR_SLAB_MINIP"), define("SVR_SLAB_MEAN")) == (1, 2, 3)
    assert abi.SLICE_COLOR_TF == define("SVR_SLICE_COLOR_TF") == 1
    assert abi.SLICE_MAX_SAMPLES == define("SVR_SLICE_MAX_SAMPLES") == sr.MAX_SAMPLES
    assert (sr.MIP, sr.MINIP, sr.MEAN) == (abi.SLAB_MIP, abi.SLAB_MINIP, abi.SLAB_MEAN)


def test_prototypes_and_defaults():
    for name in ("svr_slice_params_default", "svr_slice_params_axis", "svr_render_slice", "svr_render_slice_stack"):
        assert name in abi.PROTOTYPES and re.search(rf"\bint {name}\(", HEADER), name
    res, args = abi.PROTOTYPES["svr_render_slice_stack"]
    assert res is C.c_int and len(args) == 8 and args[6] is C.c_uint32 and args[7] is C.c_float
    assert abi.PROTOTYPES["svr_render_slice"][1] == args[:6]
    lib = abi.load()
    p = abi.SliceParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert lib.svr_slice_params_default(C.byref(p)) == 0               # plain host code: no GPU needed
    assert p.as_dict() == {"center": (0.0, 0.0, 0.0), "u": (1.0, 0.0, 0.0), "v": (0.0, 1.0, 0.0), "thickness": 0.0, "step": 1.0,
                           "mode": abi.SLAB_MIP, "flags": 0, "window_lo": 0.0, "window_hi": 1.0}


# ---------------------------------------------------------------- svr_slice_params_axis
def _aniso_volume():
    """40 x 56 x 48 voxels, spacing 1 / 0.8 / 1.3, clip members inside the volume."""
    vol = host.create_device_volume(1, (40, 56, 48), (1.0, 0.8, 1.3), 1.0)
    vol.x_clip, vol.y_clip, vol.z_clip = abi.vec2(-0.5, 0.6), abi.vec2(-1.0, 0.9), abi.vec2(-0.7, 0.4)
    return vol


@pytest.mark.parametrize("size", [(64, 48), (50, 90), (33, 33)])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_params(axis, size):
    lib = abi.load()
    lib.svr_set_error_mode(0)
    vol = _aniso_volume()
    lo, hi = sr.box(vol)
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    assert np.all(hi > lo) and not np.allclose(hi - lo, (hi - lo)[0])
    w, h = size
    for pos in (0.0, 0.25, 0.5, 1.0):
        p = host.slice_params_axis(lib, vol, axis, pos, w, h)
        d = p.as_dict()
        u, v, c = (np.array(d[k], dtype=np.float64) for k in ("u", "v", "center"))
        n = np.array(sr.normal(p.u, p.v), dtype=np.float64)
        others = [a for a in range(3) if a != axis]
        assert abs(abs(n[axis]) - 1.0) < 1e-6 and np.all(n[others] == 0), (axis, n)
        assert np.dot(u, v) == 0 and np.linalg.norm(u) == np.linalg.norm(v) > 0
        assert d["thickness"] == 0 and d["flags"] == 0 and (d["window_lo"], d["window_hi"]) == (0.0, 1.0) and d["step"] > 0
        # position 0 / 1 on the clipped faces, in between proportionally
        want = lo[axis] + pos * (hi[axis] - lo[axis])
        assert c[axis] == pytest.approx(want, abs=1e-5)
        if pos in (0.0, 1.0):
            assert c[axis] == (lo[axis] if pos == 0.0 else hi[axis])
        # the four corners of the box face land inside the image: pixel coordinates from c + u (px - w / 2) + v (py - h / 2)
        uu, vv = np.dot(u, u), np.dot(v, v)
        pxs, pys = [], []
        for ca in (lo, hi):
            for cb in (lo, hi):
                corner = c.copy()
                corner[others[0]], corner[others[1]] = ca[others[0]], cb[others[1]]
                pxs.append(np.dot(corner - c, u) / uu + 0.5 * w)
                pys.append(np.dot(corner - c, v) / vv + 0.5 * h)
        eps = 1e-4
        assert min(pxs) >= -eps and max(pxs) <= w + eps and min(pys) >= -eps and max(pys) <= h + eps, (pxs, pys)
        # fitted: the face touches the image border along one direction, and is centred
        assert (max(pxs) - min(pxs) == pytest.approx(w, abs=1e-3)) or (max(pys) - min(pys) == pytest.approx(h, abs=1e-3))
        assert min(pxs) + max(pxs) == pytest.approx(w, abs=1e-3) and min(pys) + max(pys) == pytest.approx(h, abs=1e-3)
    # refusals of the helper
    p = abi.SliceParams()
    for args in ((3, 0.5, w, h), (-1, 0.5, w, h), (0, -0.1, w, h), (0, 1.5, w, h), (0, float("nan"), w, h), (0, 0.5, 0, h), (0, 0.5, w, 0)):
        assert lib.svr_slice_params_axis(C.byref(p), C.byref(vol), args[0], C.c_float(args[1]), args[2], args[3]) != 0, args
        lib.svr_clear_error()
    assert lib.svr_slice_params_axis(None, C.byref(vol), 0, C.c_float(0.5), w, h) != 0
    lib.svr_clear_error()


# ---------------------------------------------------------------- properties of the reference
def _oblique(R, sc, w, h, thickness=0.0, step=1.0, mode=sr.MIP):
    """A plane tilted 30 degrees about the x axis through the volume's centre, pixels small enough that part of the image misses the box."""
    ext = float(sc.dim[0] * sc.spacing[0])
    px = 1.4 * ext / w
    c30, s30 = np.cos(np.pi / 6), np.sin(np.pi / 6)
    p = abi.SliceParams()
    p.center = abi.vec3(0.0, 0.0, 0.0)
    p.u = abi.vec3(px, 0.0, 0.0)
    p.v = abi.vec3(0.0, -px * c30, px * s30)
    p.thickness, p.step, p.mode, p.flags, p.window_lo, p.window_hi = thickness, step, mode, 0, 0.0, 1.0
    return p


@pytest.mark.parametrize("name", ["tiny", "tiny_head"])
def test_reference_properties(name, oracle):
    sc = scenes.make_scene(name)
    R = sr.reference(name, lambda: sc)
    w, h = 48, 40
    vals = {}
    for mode in (sr.MIP, sr.MEAN, sr.MINIP):
        p = _oblique(R, sc, w, h, thickness=6.0, step=1.5, mode=mode)
        img, cnt, M = R.image(p, w, h)
        vals[mode] = M
        hit = ~np.isnan(M)
        assert hit.any() and (~hit).any(), "hit and miss pixels must both exist"
        assert not img[~hit].any() and np.all(img[hit][:, 3] == 255)
        assert np.all(img[..., 0] == img[..., 1]) and np.all(img[..., 1] == img[..., 2])
        assert cnt["raycast_steps"] == cnt["vol_taps"] == int(R.samples(p, w, h).inside.sum()) > 0
    hit = ~np.isnan(vals[sr.MIP])
    assert np.array_equal(hit, ~np.isnan(vals[sr.MEAN])) and np.array_equal(hit, ~np.isnan(vals[sr.MINIP]))
    assert np.all(vals[sr.MIP][hit] >= vals[sr.MEAN][hit]) and np.all(vals[sr.MEAN][hit] >= vals[sr.MINIP][hit])
    assert (vals[sr.MIP][hit] > vals[sr.MINIP][hit]).any()
    # a slab of thickness 0 is the single plane, whatever step and mode say
    plane = R.image(_oblique(R, sc, w, h), w, h)
    for mode in (sr.MIP, sr.MEAN, sr.MINIP):
        other = R.image(_oblique(R, sc, w, h, thickness=0.0, step=0.37, mode=mode), w, h)
        assert np.array_equal(plane[0], other[0]) and np.array_equal(plane[2], other[2], equal_nan=True)
    assert R.samples(_oblique(R, sc, w, h), w, h).inside.shape[0] == 1
    # MIP grows and MinIP shrinks with the thickness when the thinner slab's samples are a subset: thickness T, step s has the offsets
    # j s - T / 2; thickness T + 2 s, same step, has j s - T / 2 - s, i.e. the same points and one more on either side (all exact in
    # float32 for these values)
    thin = {m: R.image(_oblique(R, sc, w, h, thickness=4.0, step=1.0, mode=m), w, h)[2] for m in (sr.MIP, sr.MINIP)}
    thick = {m: R.image(_oblique(R, sc, w, h, thickness=6.0, step=1.0, mode=m), w, h)[2] for m in (sr.MIP, sr.MINIP)}
    d_thin = (np.arange(5, dtype=np.float32) * f32(1.0)) - f32(2.0)
    d_thick = (np.arange(7, dtype=np.float32) * f32(1.0)) - f32(3.0)
    assert set(d_thin.tolist()) <= set(d_thick.tolist())
    both = ~np.isnan(thin[sr.MIP])
    assert both.any() and np.all(~np.isnan(thick[sr.MIP][both]))
    assert np.all(thick[sr.MIP][both] >= thin[sr.MIP][both]) and np.all(thick[sr.MINIP][both] <= thin[sr.MINIP][both])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_plane_on_a_voxel_layer_returns_the_raw_voxels(axis, oracle):
    """One pixel per voxel on a voxel-centre layer of the 32^3 sphere: the sampler's cell coordinates are exact integers, every lerp
    weight is 0, and the slice is the layer itself: vox * (1 / 65535) * densityScale."""
    lib = abi.load()
    lib.svr_set_error_mode(0)
    sc = scenes.make_scene("tiny", density_scale=1.75)
    R = sr.reference("tiny_ds175", lambda: sc)
    n = 32
    assert sc.dim == (n, n, n) and tuple(sc.spacing) == (1.0, 1.0, 1.0) and sc.clip == ((-1.0, 1.0),) * 3
    layer = 11
    p = host.slice_params_axis(lib, R.vol, axis, (layer + 0.5) / n, n, n)
    assert p.step == 1.0 and p.thickness == 0.0
    # the precondition, asserted: xb = fma((p - vmin) * invSize, N, -0.5) is an integer for every sample
    P, inside = R.points(p, n, n)
    assert inside.all()
    bb = R.vol.bbox
    vmin = np.array([bb.vmin.x, bb.vmin.y, bb.vmin.z], dtype=np.float32)
    inv = np.array([bb.invSize.x, bb.invSize.y, bb.invSize.z], dtype=np.float32)
    u = ((P[0] - vmin) * inv).astype(np.float32)
    xb = (u.astype(np.float64) * n - 0.5).astype(np.float32)            # exact product in double, one rounding: the fma
    assert np.array_equal(xb, np.round(xb)) and xb.min() == 0 and xb.max() == n - 1
    idx = xb.astype(np.int64)                                            # [y][x] -> (i, j, k)
    assert np.all(idx[..., axis] == layer)
    want = (sc.vox[idx[..., 2], idx[..., 1], idx[..., 0]].astype(np.float32) * f32(1.5259021896696422e-05)) * f32(sc.density_scale)
    _, _, M = R.image(p, n, n)
    assert np.array_equal(M, want)
    assert len(np.unique(M)) > 4, "the layer cuts the sphere"
    # orientation: image right / down are +y / -z, +x / -z, +x / -y
    right, down = ((1, 2), (0, 2), (0, 1))[axis]
    assert np.all(np.diff(idx[..., right], axis=1) == 1) and np.all(np.diff(idx[..., down], axis=0) == -1)


# ---------------------------------------------------------------- the skipping argument, min side
def _minmax_tables(vox, shift):
    """numpy restatement of k_minmax (csrc/svr_accel.hip): per axis, macro-cell m of S = 2^shift cells covers the voxels
    [m S - 1, m S + S - 1] (voxel -1 and voxel N are border texels = 0), the LAST macro-cell one more (border voxel N)."""
    S = 1 << shift
    lo = hi = np.pad(vox.astype(np.int64), 1)                    # index v + 1 = voxel v, v = -1 .. N
    for axis in range(3):
        n = vox.shape[axis]
        g = ((n - 1) >> shift) + 1
        los, his = [], []
        for m in range(g):
            a, b = m * S - 1, m * S + S - 1 + (1 if m == g - 1 else 0)
            b = min(b, n)                                        # voxels beyond N are border texels too
            sl = [slice(None)] * 3
            sl[axis] = slice(a + 1, b + 2)
            los.append(lo[tuple(sl)].min(axis=axis))
            his.append(hi[tuple(sl)].max(axis=axis))
        lo, hi = np.stack(los, axis=axis), np.stack(his, axis=axis)
    return lo, hi                                                # [gz][gy][gx]


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("name", ["tiny_head", "tiny_bone", "tiny_head_noisy"])
def test_fetch_stays_above_macro_cell_minimum(name, shift, oracle):
    """For 10^5 random points of the box, I(rmin) <= volume(p) for the macro-cell of the point's trilinear cell (what slab MinIP
    skips on), and a macro-cell whose rmax is 0 samples to exactly 0 (what slab MEAN and single planes skip on)."""
    sc = scenes.make_scene(name)
    R = sr.reference(name, lambda: sc)
    rmin, rmax = _minmax_tables(sc.vox, shift)
    nz, ny, nx = sc.vox.shape
    bb = R.vol.bbox
    vmin = np.array([bb.vmin.x, bb.vmin.y, bb.vmin.z], dtype=np.float32)
    vmax = np.array([bb.vmax.x, bb.vmax.y, bb.vmax.z], dtype=np.float32)
    inv = np.array([bb.invSize.x, bb.invSize.y, bb.invSize.z], dtype=np.float32)
    rng = np.random.default_rng(11 + shift)
    P = (vmin + (vmax - vmin) * rng.random((100000, 3), dtype=np.float32)).astype(np.float32)
    P[:3000] = np.where(rng.random((3000, 3)) < 0.5, vmin, vmax)                      # corners, edges and faces too
    P[3000:6000, 1] = vmin[1]
    P[6000:9000, 0] = vmax[0]
    u = ((P - vmin) * inv).astype(np.float32)
    N = np.array([nx, ny, nz], dtype=np.float64)
    xb = (u.astype(np.float64) * N - 0.5).astype(np.float32)     # the product is exact in double: one rounding, like the fma
    ux = np.floor(xb).astype(np.int64) + 1
    assert np.all((ux >= 0) & (ux <= N.astype(np.int64)))
    g = np.array([rmax.shape[2], rmax.shape[1], rmax.shape[0]])
    q = np.minimum(ux >> shift, g - 1)
    lo_raw, hi_raw = rmin[q[:, 2], q[:, 1], q[:, 0]], rmax[q[:, 2], q[:, 1], q[:, 0]]
    ds = f32(sc.density_scale)
    k = f32(1.5259021896696422e-05)
    I_lo = (lo_raw.astype(np.float32) * k) * ds
    buf = (C.c_float * 3)()
    fetch, ptr = R.lib.svo_volume_intensity, R.ptr
    I = np.empty(len(P), dtype=np.float32)
    for i, (a, b, c) in enumerate(P.tolist()):
        buf[0], buf[1], buf[2] = a, b, c
        I[i] = fetch(ptr, buf)
    bad = I < I_lo
    assert not bad.any(), f"{int(bad.sum())} violations, first at {P[bad][0]}: {I[bad][0]} < {I_lo[bad][0]}"
    assert (lo_raw > 0).any(), "macro-cells with a positive minimum exist: the bound is not vacuous"
    assert np.all(I[hi_raw == 0] == 0)
