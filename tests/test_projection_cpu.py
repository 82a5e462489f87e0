"""svr_render_projection without a GPU: the ABI of the new struct, properties of the test-side reference (tests/projection_ref.py),
and the skipping argument of csrc/svr_march.hpp checked directly against the oracle's sampler."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, scenes
from tests import projection_ref as pr

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
f32 = np.float32


# ---------------------------------------------------------------- ABI
def test_struct_layout_matches_header():
    m = re.search(r"typedef struct svr_projection_params \{(.*?)\} svr_projection_params;", HEADER, flags=re.S)
    assert m, "svr_projection_params is not declared in include/svr_abi.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(n.strip(), ctype[typ]) for n in names.split(",")]
    assert [n for n, _ in fields] == ["mode", "flags", "iso", "window_lo", "window_hi"]
    assert [(n, t) for n, t in abi.ProjectionParams._fields_] == fields
    off = 0
    for n, t in fields:                      # 4-byte members: no padding
        assert getattr(abi.ProjectionParams, n).offset == off, n
        off += C.sizeof(t)
    assert C.sizeof(abi.ProjectionParams) == off == 20
    assert abi.svr_projection_params is abi.ProjectionParams


def test_constants_match_header():
    def define(name):
        m = re.search(rf"#define\s+{name}\s+(\d+)u?\b", HEADER)
        assert m, name
        return int(m.group(1))

    assert (abi.PROJ_MIP, abi.PROJ_MEAN, abi.PROJ_ISO) == (define("SVR_PROJ_MIP"), define("SVR_PROJ_MEAN"), define("SVR_PROJ_ISO")) == (1, 2, 3)
    assert abi.PROJ_COLOR_TF == define("SVR_PROJ_COLOR_TF") == 1
    assert (pr.MIP, pr.MEAN, pr.ISO) == (abi.PROJ_MIP, abi.PROJ_MEAN, abi.PROJ_ISO)


def test_prototypes_and_defaults():
    assert "svr_render_projection" in abi.PROTOTYPES and "svr_projection_params_default" in abi.PROTOTYPES
    res, args = abi.PROTOTYPES["svr_render_projection"]
    assert res is C.c_int and len(args) == 6 and args[4] is C.c_float
    lib = abi.load()
    p = abi.ProjectionParams(-1, 99, 9.0, 9.0, 9.0)
    assert lib.svr_projection_params_default(C.byref(p)) == 0          # plain host code: no GPU needed
    assert p.as_dict() == {"mode": abi.PROJ_MIP, "flags": 0, "iso": 0.5, "window_lo": 0.0, "window_hi": 1.0}


# ---------------------------------------------------------------- properties of the reference
@pytest.mark.parametrize("name", ["tiny", "tiny_head"])
def test_reference_properties(name, oracle):
    sc = scenes.make_scene(name)
    R = pr.reference(name, lambda: sc)
    step = sc.step_size()
    rays = R.rays(step)
    hits = [(x, y, rays[y][x]) for y in range(sc.height) for x in range(sc.width) if rays[y][x] is not None]
    assert 0 < len(hits) < sc.width * sc.height, "the scene must have hit and miss pixels"
    img_mip, c_mip, M_mip = R.image(pr.MIP, step)
    img_mean, c_mean, M_mean = R.image(pr.MEAN, step)
    n_samples = sum(len(r.Is) for _, _, r in hits)
    assert c_mip == c_mean == {"raycast_steps": n_samples, "vol_taps": n_samples}
    for x, y, r in hits:
        assert len(r.Is) >= 1 and np.all(np.diff(r.ts) > 0)
        M = M_mip[y, x]
        assert np.all(M >= r.Is) and (M == 0 or np.any(r.Is == M))
        assert r.Is.min() <= M_mean[y, x] <= r.Is.max()
        assert tuple(img_mip[y, x, :3]) == (img_mip[y, x, 0],) * 3 and img_mip[y, x, 3] == 255 and img_mean[y, x, 3] == 255
    # miss pixels are (0, 0, 0, 0) in every mode
    miss = np.array([[rays[y][x] is None for x in range(sc.width)] for y in range(sc.height)])
    iso = 0.3
    img_iso, c_iso, ns = R.image(pr.ISO, step, iso=iso)
    for img in (img_mip, img_mean, img_iso):
        assert not img[miss].any()
    assert np.all(ns[miss] == -2) and not img_iso[ns == -1].any() and np.all(img_iso[ns >= 0][:, 3] == 255)
    assert (ns >= 0).any() and (ns == -1).any()
    # the bracket of the bisection
    bisected = 0
    for x, y, r in hits:
        res = R.iso_search(r, iso)
        if res is None:
            assert np.all(r.Is < f32(iso))
            continue
        n, lo, hi, I_hi = res
        assert n == ns[y, x] and np.all(r.Is[:n] < f32(iso)) and r.Is[n] >= f32(iso)
        assert I_hi >= f32(iso) and R.intensity(R.point(r, hi)) == I_hi
        if n == 0:
            assert lo is None and hi == r.ts[0]
            continue
        bisected += 1
        assert R.intensity(R.point(r, lo)) < f32(iso)
        assert r.ts[n - 1] <= lo < hi <= r.ts[n]
        width = (np.float64(r.ts[n]) - np.float64(r.ts[n - 1])) * 2.0 ** -8
        assert np.float64(hi) - np.float64(lo) <= width + np.float64(np.spacing(hi)), (x, y, lo, hi)
    assert bisected > 0


# ---------------------------------------------------------------- the skipping argument
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
def test_fetch_stays_within_macro_cell_bounds(name, shift, oracle):
    """For 10^5 random points of the box, volume(p) lies within [I(rmin), I(rmax)] of the macro-cell of its trilinear cell."""
    sc = scenes.make_scene(name)
    R = pr.reference(name, lambda: sc)
    rmin, rmax = _minmax_tables(sc.vox, shift)
    nz, ny, nx = sc.vox.shape
    bb = R.o.s.vol.bbox
    vmin = np.array([bb.vmin.x, bb.vmin.y, bb.vmin.z], dtype=np.float32)
    vmax = np.array([bb.vmax.x, bb.vmax.y, bb.vmax.z], dtype=np.float32)
    inv = np.array([bb.invSize.x, bb.invSize.y, bb.invSize.z], dtype=np.float32)
    rng = np.random.default_rng(7 + shift)
    P = (vmin + (vmax - vmin) * rng.random((100000, 3), dtype=np.float32)).astype(np.float32)
    P[:3000] = np.where(rng.random((3000, 3)) < 0.5, vmin, vmax)                      # corners, edges and faces too
    P[3000:6000, 0] = vmin[0]
    P[6000:9000, 2] = vmax[2]
    # the sampler's cell (cell_of): u = (p - vmin) * invSize, xb = fma(u, N, -0.5), c = floor(xb)
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
    I_hi = (hi_raw.astype(np.float32) * k) * ds
    buf = (C.c_float * 3)()
    fetch, ptr = R.lib.svo_volume_intensity, R.ptr
    I = np.empty(len(P), dtype=np.float32)
    for i, (a, b, c) in enumerate(P.tolist()):
        buf[0], buf[1], buf[2] = a, b, c
        I[i] = fetch(ptr, buf)
    bad = (I < I_lo) | (I > I_hi)
    assert not bad.any(), f"{int(bad.sum())} violations, first at {P[bad][0]}: {I[bad][0]} outside [{I_lo[bad][0]}, {I_hi[bad][0]}]"
    assert (hi_raw == 0).any() == (name != "tiny_head_noisy"), "exactly empty macro-cells exist unless the air is noisy"
    assert np.all(I[hi_raw == 0] == 0)
