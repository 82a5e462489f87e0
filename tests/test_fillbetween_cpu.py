"""Fill between slices without a GPU (include/svr_abi.h, "fill between slices"): the numpy reference against scipy's 2D
distance transform, the properties of the rule (reversal, a cone between two concentric discs, the tie against an empty key, the known
limit), every refusal of the three calls -- they stand before the device is touched -- and the Python layer on the fake device."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import fillbetween_ref as fr
from tests.host_fake import FakeDevice

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
MASK = 1 << 40           # any non-null "device pointer": a refused call does not touch it


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    return lib


def disc(nv, nu, cu, cv, r):
    v, u = np.mgrid[:nv, :nu]
    return (u - cu) ** 2 + (v - cv) ** 2 <= r * r


# ------------------------------------------------------------------------------------------------ the reference
def test_structs_and_constants(lib):
    assert C.sizeof(abi.FillBetweenParams) == 32 and abi.FillBetweenParams.keys.offset == 24
    assert C.sizeof(abi.FillBetweenInfo) == 56 and abi.FillBetweenInfo.voxels_in.offset == 32
    for name, value in (("SVR_FILL_KEEP_BETWEEN", abi.FILL_KEEP_BETWEEN), ("SVR_FILL_GAP_BY_GAP", abi.FILL_GAP_BY_GAP),
                        ("SVR_FILL_MAP_BUDGET_BYTES", abi.FILL_MAP_BUDGET_BYTES)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)u", HEADER).group(1)) == value
    p = abi.FillBetweenParams(7, 7, (7, 7, 7), 7)
    assert lib.svr_fill_between_params_default(C.byref(p)) == 0
    assert (p.axis, p.flags, list(p.weights), p.nkeys, bool(p.keys)) == (2, 0, [0, 0, 0], 0, False)


@pytest.mark.parametrize("weights", [None, (4, 1, 9), (1, 16, 2)])
def test_reference_planar_maps_are_scipy_edt(weights):
    """round(distance_transform_edt(s)^2) on the set voxels and of ~s on the unset ones, per 2D slice, with sampling = sqrt(w)"""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    m = rng.random((6, 9, 13)) < 0.4
    m[2] = disc(9, 13, 6, 4, 3.3)
    m[3], m[4] = False, True                                  # a slice without a set voxel, one without an unset voxel: SVR_DIST_NONE
    for axis in range(3):
        wu, wv = fr.planar_weights(axis, weights)
        got = fr.slice_distance(m, axis, weights)
        for k, s in enumerate(fr.planes(m, axis)):
            if s.all() or not s.any():
                assert (got[k] == fr.NONE).all()
                continue
            sampling = (math.sqrt(wv), math.sqrt(wu))
            want = np.where(s, ndi.distance_transform_edt(s, sampling=sampling), ndi.distance_transform_edt(~s, sampling=sampling)) ** 2
            assert np.array_equal(got[k], np.rint(want).astype(np.uint32)), (axis, k)
    assert np.array_equal(fr.slice_distance(m, 1, weights, [4, 0, 4]), fr.slice_distance(m, 1, weights)[[4, 0, 4]])
    assert [int(c) for c in fr.slice_counts(m, 0)] == [int(m[:, :, x].sum()) for x in range(13)]


def test_reversing_the_slices_reverses_the_result():
    rng = np.random.default_rng(1)
    m = np.zeros((9, 7, 11), bool)
    for k in (0, 3, 8):
        m[k] = rng.random((7, 11)) < 0.5
    for keep in (False, True):
        m[5] = rng.random((7, 11)) < 0.2 if keep else False
        for axis in range(3):
            src = np.ascontiguousarray(np.moveaxis(m, 0, 2 - axis))       # the keyed axis becomes `axis`
            a, _ = fr.fill_between(src, axis, [0, 3, 8] if keep else None, (4, 1, 9), keep)
            flipped = np.ascontiguousarray(np.flip(src, 2 - axis))
            b, _ = fr.fill_between(flipped, axis, [0, 5, 8] if keep else None, (4, 1, 9), keep)
            assert np.array_equal(np.flip(a, 2 - axis), b), (axis, keep)


def test_cone_between_two_concentric_discs():
    """Discs of radius 15.3 and 4.2 twelve slices apart: slice t is the disc of radius ((n - t) r0 + t r1) / n.  A voxel is misjudged
    only if its two planar distances are off by enough to move the zero of the interpolated signed distance past it; the planar maps
    measure to voxel centres of the other kind rather than to the circle, which is off by less than one voxel spacing, so the radial
    error stays below one voxel (measured: 0.49)."""
    n, r0, r1, c = 12, 15.3, 4.2, 20
    m = np.zeros((n + 1, 41, 41), bool)
    m[0], m[n] = disc(41, 41, c, c, r0), disc(41, 41, c, c, r1)
    out, info = fr.fill_between(m, 2)
    assert (info["keys"], info["gaps"], info["filled_slices"]) == (2, 1, n - 1)
    v, u = np.mgrid[:41, :41]
    rr = np.hypot(u - c, v - c)
    worst = 0.0
    for t in range(1, n):
        r = ((n - t) * r0 + t * r1) / n
        worst = max(worst, float((rr[out[t]] - r).max()), float((r - rr[~out[t]]).max()))
    print("cone: worst radial error", worst)
    assert worst < 1.0


def test_full_key_against_empty_key_is_the_tie_rule():
    m = np.zeros((7, 4, 5), bool)
    m[0] = True
    out, info = fr.fill_between(m, 2, [0, 6])
    assert [bool(s.all()) for s in out] == [True, True, True, False, False, False, False] and not out[3:].any()     # t = 3 = n / 2: unset
    assert (info["gaps"], info["filled_slices"], info["voxels_out"]) == (1, 5, 60)
    out, _ = fr.fill_between(m, 2)                              # one key: nothing to do
    assert np.array_equal(out, m)


def test_known_limit_disjoint_shapes_fade():
    """the figures of the header: discs of radius 6 whose centres lie 20 voxels apart, eight slices apart"""
    m = np.zeros((9, 31, 61), bool)
    m[0], m[8] = disc(31, 61, 15, 15, 6), disc(31, 61, 35, 15, 6)
    out, _ = fr.fill_between(m, 2)
    counts = [int(c) for c in fr.slice_counts(out, 2)]
    assert counts == [113, 59, 8, 0, 0, 0, 8, 59, 113]
    assert ", ".join(str(c) for c in counts) in re.sub(r"\s*\n \*\s*", " ", HEADER)


# ------------------------------------------------------------------------------------------------ the refusals
def refused(lib, rc, code):
    assert rc == code and lib.svr_last_error_code() == code, (rc, lib.svr_last_error())
    lib.svr_clear_error()


def test_slice_counts_refusals(lib):
    counts = (C.c_uint64 * 8)()
    refused(lib, lib.svr_region_slice_counts(None, 4, 4, 4, 2, counts), -4)
    refused(lib, lib.svr_region_slice_counts(MASK, 4, 4, 4, 2, None), -4)
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (2048, 2048, 513)):
        refused(lib, lib.svr_region_slice_counts(MASK, *dims, 2, counts), -6)
    for axis in (-1, 3):
        refused(lib, lib.svr_region_slice_counts(MASK, 4, 4, 4, axis, counts), -3)


def test_slice_distance_refusals(lib):
    u32, i32 = lambda *v: (C.c_uint32 * len(v))(*v), lambda *v: (C.c_int32 * len(v))(*v)      # noqa: E731
    call = lib.svr_region_slice_distance
    refused(lib, call(None, 4, 4, 4, 2, None, None, 0, MASK), -4)
    refused(lib, call(MASK, 4, 4, 4, 2, None, None, 0, None), -4)
    for dims in ((0, 4, 4), (4, 4, -3), (2048, 2048, 513)):
        refused(lib, call(MASK, *dims, 2, None, None, 0, MASK), -6)
    for axis in (-1, 3):
        refused(lib, call(MASK, 4, 4, 4, axis, None, None, 0, MASK), -3)
    for w in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):                 # every weight is at least 1, the unused one too
        refused(lib, call(MASK, 4, 4, 4, 2, u32(*w), None, 0, MASK), -3)
    # wu (nu - 1)^2 + wv (nv - 1)^2 > 0xFFFFFFFE; the slicing axis's length and weight take no part
    refused(lib, call(MASK, 65537, 2, 2, 2, None, None, 0, MASK), -3)
    refused(lib, call(MASK, 2001, 2, 2, 1, u32(1074, 1, 1), None, 0, MASK), -3)
    refused(lib, call(MASK, 3, 65536, 400, 0, None, None, 0, MASK), -3)                      # 65535^2 + 399^2
    refused(lib, call(MASK, 65537, 4, 4, 0, None, None, 0, MASK), -3)                        # more than 65536 slices
    for slices, n in ((i32(0, 1), 0), (i32(0, 1), -2), (i32(0, 4), 2), (i32(-1, 1), 2)):
        refused(lib, call(MASK, 4, 4, 4, 2, None, slices, n, MASK), -3)


def test_fill_between_refusals(lib):
    i32 = lambda *v: (C.c_int32 * len(v))(*v)                   # noqa: E731
    info = abi.FillBetweenInfo()

    def call(dims=(4, 4, 8), params=True, mask=MASK, out=MASK, **kw):
        p = abi.FillBetweenParams()
        lib.svr_fill_between_params_default(C.byref(p))
        keys = kw.pop("keys", None)
        if keys is not None:
            p.keys, p.nkeys = keys, kw.pop("nkeys", len(keys))
        for name, value in kw.items():
            setattr(p, name, value)
        return lib.svr_region_fill_between(mask, *dims, C.byref(p) if params else None, out, C.byref(info))

    refused(lib, call(mask=None), -4)
    refused(lib, call(out=None), -4)
    refused(lib, call(params=False), -4)
    for dims in ((0, 4, 4), (4, 4, -3), (2048, 2048, 513)):
        refused(lib, call(dims), -6)
    for axis in (-1, 3):
        refused(lib, call(axis=axis), -3)
    for w in ((0, 1, 1), (1, 0, 1), (3, 1, 0)):                 # 0, 0, 0 is 1, 1, 1; a single 0 is refused
        refused(lib, call(weights=(C.c_uint32 * 3)(*w)), -3)
    refused(lib, call((65537, 2, 2)), -3)
    refused(lib, call((2001, 2, 4), weights=(C.c_uint32 * 3)(1074, 1, 1)), -3)
    refused(lib, call((65537, 4, 4), axis=0), -3)
    for keys in (i32(0, 0), i32(3, 2), i32(0, 8), i32(-1, 4), i32(0, 2, 2, 5)):
        refused(lib, call(keys=keys), -3)
    refused(lib, call(keys=i32(0, 4), nkeys=-1), -3)
    for flags in (4, 0x80000000, 7):
        refused(lib, call(flags=flags), -3)
    refused(lib, lib.svr_region_fill_between_last_ms(None), -4)
    refused(lib, lib.svr_fill_between_params_default(None), -4)
    assert lib.svr_region_fill_between_pass_ms(None, None, None) == 0


# ------------------------------------------------------------------------------------------------ the Python layer on the fake device
def raises_before_any_call(fn, *args, **kw):
    dev = FakeDevice()
    with pytest.raises(ValueError):
        getattr(dev, fn)(*args, **kw)
    assert dev.lib.calls == [] and dev.live == set() and dev.nmalloc == 0


def test_python_argument_errors():
    m = np.zeros((6, 4, 5), bool)
    E = raises_before_any_call
    for fn in ("region_slice_counts", "region_slice_distance", "region_fill_between"):
        E(fn, m, 3)
        E(fn, m, -1)
        E(fn, np.zeros((4, 5), bool))
        E(fn, 1 << 61)                                          # a device pointer without shape=
    E("region_slice_distance", m, 2, slices=[])
    E("region_slice_distance", m, 2, slices=[6])
    E("region_slice_distance", m, 0, slices=[5])
    E("region_slice_distance", m, 2, slices=[-1])
    for keys in ([0, 0], [3, 2], [0, 6], [-1, 2]):
        E("region_fill_between", m, 2, keys)
    E("region_fill_between", m, 0, [0, 5])
    for w in ((0, 1, 1), (1, 1), (1, 1, -2)):
        E("region_fill_between", m, 2, None, w)


def test_fake_device_calls_and_no_leak():
    m = np.zeros((6, 4, 40), bool)
    dev = FakeDevice()
    counts = dev.region_slice_counts(m, 1)
    assert counts.shape == (4,) and counts.dtype == np.uint64 and dev.live == set()
    assert dev.lib.calls[-1]["fn"] == "svr_region_slice_counts" and dev.lib.calls[-1]["args"][1:5] == [40, 4, 6, 1]
    maps = dev.region_slice_distance(m, 0, (4, 1, 9), slices=[39, 0, 39])
    assert maps.shape == (3, 6, 4) and maps.dtype == np.uint32 and dev.live == set()
    call = dev.lib.calls[-1]
    assert call["fn"] == "svr_region_slice_distance" and call["args"][1:5] == [40, 4, 6, 0] and call["args"][7] == 3
    assert dev.region_slice_distance(m, 2).shape == (6, 4, 40) and dev.lib.calls[-1]["args"][5:8] == [None, None, 6]
    assert dev.region_slice_distance(m, 1).shape == (4, 6, 40)
    out, info = dev.region_fill_between(m, 2, [0, 3, 5], (4, 1, 9), keep_between=True)
    assert out.shape == m.shape and isinstance(info, abi.FillBetweenInfo) and dev.live == set()
    call = dev.lib.calls[-1]
    assert call["fn"] == "svr_region_fill_between" and call["args"][1:4] == [40, 4, 6]
    p = call["args"][4]
    assert (p["axis"], p["flags"], p["weights"], p["nkeys"]) == (2, abi.FILL_KEEP_BETWEEN, [4, 1, 9], 3) and p["keys"] is not None
    dev.region_fill_between(m, 0, gap_by_gap=True)
    p = dev.lib.calls[-1]["args"][4]
    assert (p["axis"], p["flags"], p["weights"], p["nkeys"], p["keys"]) == (0, abi.FILL_GAP_BY_GAP, [0, 0, 0], 0, None)
    assert dev.region_fill_between_last_ms() == 0.0 and dev.region_fill_between_pass_ms() == (0.0, 0.0, 0.0)
    # nothing stays allocated when the library call or an allocation fails
    for fn, args in (("region_slice_counts", (m, 2)), ("region_slice_distance", (m, 2)), ("region_fill_between", (m, 2, [0, 4]))):
        for fail in (dict(fail_call=1), dict(fail_malloc=1), dict(fail_malloc=2)):
            dev = FakeDevice()
            dev.lib.fail_call, dev.fail_malloc = fail.get("fail_call"), fail.get("fail_malloc")
            if fn == "region_slice_counts" and fail.get("fail_malloc") == 2:
                continue                                       # (it allocates once)
            with pytest.raises(host.SvrError):
                getattr(dev, fn)(*args)
            assert dev.live == set()
