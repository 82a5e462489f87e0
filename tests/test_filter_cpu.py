"""The volume filters without a GPU: the test-side reference (tests/filter_ref.py) against scipy.ndimage and against cases worked out
by hand, the demonstration that motivates them (a salted head phantom whose bone window falls into 747 pieces and is one piece again
after one median pass), svr_volume_smooth_radii against its definition, the ABI of the new symbols and constants, every refusal
(arguments are checked before the device is touched) and the new arguments of examples/render_mhd.cpp."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import filter_ref as fr
from tests import label_ref
from tests.test_region_cpu import BONE
from tests.cpp_example import build_example

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
SHAPES = [(1, 1, 1), (2, 2, 2), (1, 1, 40), (3, 1, 33), (5, 7, 9)]


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    lib.svr_clear_error()
    return lib


# ---------------------------------------------------------------- the reference against scipy
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_rank_reference_against_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    for seed, vol in enumerate((fr.random_volume(shape, 11), fr.extremes_volume(shape, 12))):
        for k, element in enumerate(fr.ELEMENTS):
            fp = ndi.generate_binary_structure(3, k + 1)
            assert int(fp.sum()) == element + 1
            for op, fn in ((fr.MEDIAN, ndi.median_filter), (fr.MIN, ndi.minimum_filter), (fr.MAX, ndi.maximum_filter)):
                want = fn(vol, footprint=fp, mode="nearest")
                assert want.dtype == np.uint16 and np.array_equal(fr.rank(vol, op, element), want), (shape, seed, element, op)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_smooth_reference_against_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    vol = fr.random_volume(shape, 21)
    for radii in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (2, 3, 1), (8, 8, 8)):
        want = vol.astype(np.int64)
        for a, r in enumerate(radii):
            if r:
                w = np.array([math.comb(2 * r, k) for k in range(2 * r + 1)], dtype=np.int64)
                want = (ndi.correlate1d(want, w, axis=2 - a, mode="nearest") + (1 << (2 * r - 1))) >> (2 * r)
        assert np.array_equal(fr.smooth(vol, radii), want.astype(np.uint16)), (shape, radii)


# ---------------------------------------------------------------- by hand
def test_window_sizes_and_ranks():
    assert [len(fr.offsets(e)) for e in fr.ELEMENTS] == [7, 19, 27]
    assert [len(fr.offsets(e)) // 2 for e in fr.ELEMENTS] == [3, 9, 13]


def test_a_constant_volume_is_a_fixpoint():
    for value in (0, 1, 32768, 65535):
        vol = np.full((3, 4, 5), value, dtype=np.uint16)
        for op in fr.OPS:
            for element in fr.ELEMENTS:
                assert np.array_equal(fr.rank(vol, op, element, 2), vol)
        for radii in ((1, 0, 0), (2, 3, 1), (8, 8, 8)):
            assert np.array_equal(fr.smooth(vol, radii), vol)


def test_the_accumulator_bound():
    """All-65535 at radius 8: the sum is 65535 * 4^8 + 2^15 = 4 294 934 528, above 2^31 and below 2^32, and the result is 65535."""
    assert 65535 * 4 ** 8 + 2 ** 15 == 4294934528 and 2 ** 31 < 4294934528 < 2 ** 32
    assert sum(math.comb(16, k) for k in range(17)) == 4 ** 8
    vol = np.full((2, 3, 20), 65535, dtype=np.uint16)
    assert (fr.smooth(vol, (8, 8, 8)) == 65535).all()


def test_one_bright_voxel():
    vol = np.zeros((5, 5, 5), dtype=np.uint16)
    vol[2, 2, 2] = 65535
    for element in fr.ELEMENTS:
        assert not fr.rank(vol, fr.MEDIAN, element).any()                                 # it vanishes under the median
        assert np.array_equal(fr.rank(vol, fr.MIN, element), np.zeros_like(vol))
        grown = fr.rank(vol, fr.MAX, element)                                             # and becomes the element's shape under max
        assert int((grown == 65535).sum()) == element + 1 and int((grown == 0).sum()) == 125 - element - 1
        for dz, dy, dx in fr.offsets(element):
            assert grown[2 + dz, 2 + dy, 2 + dx] == 65535


def test_a_bright_corner_voxel_and_the_clamped_border():
    """Voxel x = 0 of a row of zeros holds 65535.  At radii (1, 0, 0) the kernel is (1, 2, 1) / 4 and the tap left of x = 0 is x = 0
    again: out[0] = (3 * 65535 + 2) >> 2 = 49151, out[1] = (65535 + 2) >> 2 = 16384, out[2] = 0."""
    vol = np.zeros((3, 3, 4), dtype=np.uint16)
    vol[0, 0, 0] = 65535
    out = fr.smooth(vol, (1, 0, 0))
    assert out[0, 0].tolist() == [49151, 16384, 0, 0] and not out[1:].any() and not out[0, 1:].any()
    assert (3 * 65535 + 2) >> 2 == 49151 and (65535 + 2) >> 2 == 16384
    # the same voxel along y and z; and under the rank filters the corner's window holds the voxel 4 / 7 / 8 times of 7 / 19 / 27
    assert fr.smooth(vol, (0, 1, 0))[0, :, 0].tolist() == [49151, 16384, 0] and fr.smooth(vol, (0, 0, 1))[:, 0, 0].tolist() == [49151, 16384, 0]
    assert fr.rank(vol, fr.MEDIAN, 6)[0, 0, 0] == 65535 and fr.rank(vol, fr.MEDIAN, 18)[0, 0, 0] == 0 and fr.rank(vol, fr.MEDIAN, 26)[0, 0, 0] == 0


def test_unsigned_order():
    """32768 and above are ordinary data: a signed 16-bit compare would call them negative."""
    vol = np.array([[[1, 40000, 2]]], dtype=np.uint16)
    assert fr.rank(vol, fr.MAX, 6)[0, 0].tolist() == [40000, 40000, 40000] and fr.rank(vol, fr.MIN, 6)[0, 0].tolist() == [1, 1, 2]


def test_iterations_compose():
    vol = fr.random_volume((4, 5, 6), 5)
    assert np.array_equal(fr.rank(vol, fr.MEDIAN, 18, 3), fr.rank(fr.rank(fr.rank(vol, fr.MEDIAN, 18), fr.MEDIAN, 18), fr.MEDIAN, 18))


# ---------------------------------------------------------------- the demonstration
def test_the_median_mends_the_salted_bone_window():
    assert BONE[:2] == fr.BONE and BONE[4] == 5410
    clean, salted = fr.heads()
    assert clean.shape == (48, 48, 48) and int((clean != salted).sum()) > 0
    bone = fr.window(clean)
    assert int(bone.sum()) == 5410 and label_ref.label(bone, 6)[1] == 1
    noisy = fr.window(salted)
    assert int(noisy.sum()) == 6191 and label_ref.label(noisy, 6)[1] == 747
    mended = fr.window(fr.cached_rank("salted", fr.MEDIAN, 18))
    assert int(mended.sum()) == 5336 and label_ref.label(mended, 6)[1] == 1
    assert int((mended ^ bone).sum()) == 270 <= 0.05 * 5410


# ---------------------------------------------------------------- svr_volume_smooth_radii
@pytest.mark.parametrize("spacing, sigma", [((1.0, 1.0, 1.0), 1.0), ((1.0, 1.0, 1.0), 2.0), ((0.7, 0.7, 1.5), 1.0), ((0.5, 1.0, 2.0), 0.9),
                                            ((1.0, 1.0, 1.0), 0.4), ((3.0, 2.0, 1.0), 0.0), ((1.0, 1.0, 1.0), 0.5), ((0.25, 0.5, 1.0), 0.5)])
def test_smooth_radii_definition(lib, spacing, sigma):
    radii, applied = host.smooth_radii(spacing, sigma, lib)
    want_r, want_s = fr.radii_from_sigma(spacing, sigma)
    assert radii == want_r and applied == pytest.approx(want_s, rel=1e-15, abs=0.0)
    if sigma == 0.0:
        assert radii == (0, 0, 0) and applied == (0.0, 0.0, 0.0)


def test_smooth_radii_by_hand(lib):
    assert host.smooth_radii((1, 1, 1), 2.0, lib)[0] == (8, 8, 8)                         # variance r / 2 = 4
    assert host.smooth_radii((1, 1, 1), 1.0, lib) == ((2, 2, 2), (1.0, 1.0, 1.0))
    assert host.smooth_radii((1, 2, 4), 2.0, lib)[0] == (8, 2, 1)                         # 2 (2 / 4)^2 = 0.5 rounds away from zero
    sigma_out = (C.c_double * 3)()
    r = (C.c_uint32 * 3)()
    assert lib.svr_volume_smooth_radii((C.c_double * 3)(1, 1, 1), 1.0, r, None) == 0 and list(r) == [2, 2, 2]     # sigma_out may be NULL
    assert lib.svr_volume_smooth_radii((C.c_double * 3)(1, 1, 1), 1.0, r, sigma_out) == 0 and list(sigma_out) == [1.0, 1.0, 1.0]


# ---------------------------------------------------------------- the ABI
def test_symbols_and_constants():
    for name in ("svr_volume_rank", "svr_volume_smooth", "svr_volume_smooth_radii", "svr_volume_filter_last_ms"):
        assert name in abi.PROTOTYPES and re.search(r"\b" + name + r"\(", HEADER), name
    for name, value in (("SVR_FILTER_MEDIAN", 1), ("SVR_FILTER_MIN", 2), ("SVR_FILTER_MAX", 3), ("SVR_FILTER_MAX_ITERATIONS", 64), ("SVR_SMOOTH_MAX_RADIUS", 8)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", HEADER), name
        assert getattr(abi, name[4:]) == value == {"SVR_FILTER_MEDIAN": fr.MEDIAN, "SVR_FILTER_MIN": fr.MIN, "SVR_FILTER_MAX": fr.MAX,
                                                   "SVR_FILTER_MAX_ITERATIONS": fr.MAX_ITERATIONS, "SVR_SMOOTH_MAX_RADIUS": fr.MAX_RADIUS}[name]
    for name in ("volume_rank", "volume_median", "volume_smooth", "volume_filter_last_ms"):
        assert callable(getattr(host.Device, name))
    assert "svr_filter.hip" in __import__("sunvolumerender_amd._build", fromlist=["HIP_SOURCES"]).HIP_SOURCES


# ---------------------------------------------------------------- refusals: all are decided before the device is touched
A, OUT = 0x10000, 0x30000                                # "device pointers": nothing is read or written through them


def _refused(lib, name, rc, code, word):
    msg = lib.svr_last_error().decode()
    last = lib.svr_last_error_code()
    lib.svr_clear_error()
    assert rc == last == code and name in msg and word in msg, (name, rc, last, msg)


DIMS = [(dict(dims=(0, 4, 4)), -6, "dimensions"), (dict(dims=(4, -1, 4)), -6, "dimensions"), (dict(dims=(4, 4, 0)), -6, "dimensions"),
        (dict(dims=(2048, 1024, 1025)), -6, "2^31"), (dict(dims=(2**16, 2**16, 1)), -6, "2^31")]
# 4 x 4 x 4 u16 are 128 bytes: an `out` that starts inside them, or they inside it, overlaps; a HOST source overlaps nothing
OVERLAPS = [(dict(out=A), -3, "overlap"), (dict(out=A + 2), -3, "overlap"), (dict(out=A + 126), -3, "overlap"), (dict(vox=OUT + 126), -3, "overlap")]


def _rank(lib, vox=A, dims=(4, 4, 4), on_dev=1, op=1, element=6, iterations=1, out=OUT):
    return lib.svr_volume_rank(C.c_void_p(vox), *dims, on_dev, op, element, iterations, C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [(dict(vox=None), -4, "null"), (dict(out=None), -4, "null"), (dict(op=0), -3, "op"), (dict(op=4), -3, "op"),
                                            (dict(element=0), -3, "element"), (dict(element=7), -3, "element"), (dict(element=27), -3, "element"),
                                            (dict(iterations=0), -3, "iterations"), (dict(iterations=65), -3, "iterations"),
                                            (dict(iterations=0xFFFFFFFF), -3, "iterations")] + DIMS + OVERLAPS)
def test_rank_refusals(lib, kw, code, word):
    _refused(lib, "svr_volume_rank", _rank(lib, **kw), code, word)


def _smooth(lib, vox=A, dims=(4, 4, 4), on_dev=1, radii=(1, 1, 1), out=OUT):
    return lib.svr_volume_smooth(C.c_void_p(vox), *dims, on_dev, None if radii is None else (C.c_uint32 * 3)(*radii), C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [(dict(vox=None), -4, "null"), (dict(out=None), -4, "null"), (dict(radii=None), -4, "null"),
                                            (dict(radii=(9, 0, 0)), -3, "radius"), (dict(radii=(0, 9, 0)), -3, "radius"), (dict(radii=(8, 8, 0xFFFFFFFF)), -3, "radius"),
                                            (dict(radii=(0, 0, 0), out=A), -3, "overlap")] + DIMS + OVERLAPS)
def test_smooth_refusals(lib, kw, code, word):
    _refused(lib, "svr_volume_smooth", _smooth(lib, **kw), code, word)


def _radii(lib, spacing=(1.0, 1.0, 1.0), sigma=1.0, outs=True):
    r = (C.c_uint32 * 3)(77, 77, 77)
    so = (C.c_double * 3)(77.0, 77.0, 77.0)
    rc = lib.svr_volume_smooth_radii(None if spacing is None else (C.c_double * 3)(*spacing), sigma, r if outs else None, so)
    assert list(r) == [77, 77, 77] and list(so) == [77.0, 77.0, 77.0]                     # nothing is written on a refusal
    return rc


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("kw, code, word", [(dict(spacing=None), -4, "null"), (dict(outs=False), -4, "null"),
                                            (dict(spacing=(0.0, 1.0, 1.0)), -3, "spacing"), (dict(spacing=(1.0, -1.0, 1.0)), -3, "spacing"),
                                            (dict(spacing=(1.0, 1.0, INF)), -3, "spacing"), (dict(spacing=(NAN, 1.0, 1.0)), -3, "spacing"),
                                            (dict(sigma=-0.5), -3, "sigma"), (dict(sigma=INF), -3, "sigma"), (dict(sigma=NAN), -3, "sigma"),
                                            (dict(sigma=2.07), -3, "radius"),                    # 2 * 2.07^2 = 8.57: radius 9
                                            (dict(sigma=1.0, spacing=(1.0, 0.4, 1.0)), -3, "radius"),   # 2 / 0.16 = 12.5 on y
                                            (dict(sigma=1e300, spacing=(1e-300, 1.0, 1.0)), -3, "radius")])
def test_smooth_radii_refusals(lib, kw, code, word):
    _refused(lib, "svr_volume_smooth_radii", _radii(lib, **kw), code, word)


def test_the_largest_admitted_sigma(lib):
    assert host.smooth_radii((1, 1, 1), 2.06, lib)[0] == (8, 8, 8)                        # 2 * 2.06^2 = 8.49


# ---------------------------------------------------------------- examples/render_mhd.cpp: the filter arguments
@pytest.fixture(scope="module")
def render_mhd(tmp_path_factory):
    exe = build_example(tmp_path_factory.mktemp("render_mhd_filter"), strict=True)
    return exe


@pytest.mark.parametrize("args", [["-median"], ["-median", "18"], ["-median", "7", "1"], ["-median", "18", "0"], ["-median", "18", "65"], ["-median", "x", "1"],
                                  ["-median", "18", "2x"], ["-median", "-6", "1"], ["-smooth"], ["-smooth", "0"], ["-smooth", "-1"], ["-smooth", "x"],
                                  ["-smooth", "1.5mm"], ["-smooth", "inf"], ["-smooth", "nan"], ["-show-filtered"], ["-show-filtered", "-threshold", "0", "10"]])
def test_render_mhd_rejects_bad_filter_arguments(render_mhd, tmp_path, args):
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), *args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.strip(), (res.returncode, res.stderr)


def test_render_mhd_usage_names_the_filter_steps(render_mhd):
    err = subprocess.run([str(render_mhd)], capture_output=True, text=True, timeout=60).stderr
    for word in ("-median E N", "-smooth SIGMA", "-show-filtered"):
        assert word in err, word
