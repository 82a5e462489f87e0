"""The comparison calls without a GPU (include/svr_abi.h, "comparing segmentations"): the numpy reference of
tests/compare_ref.py against brute force on tiny masks; the library's host code (svr_overlap_match, svr_region_compare_measure) against
the formulas of the header; every refusal, which the library answers before it touches the device; and the new Python methods on the
fake device of tests/host_fake.py, which may leave no buffer behind however a call ends."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from sunvolumerender_amd.host import SvrError
from tests import compare_ref as cr
from tests.host_fake import Dev, Out, run_row

# ---------------- the reference against brute force ----------------
TINY = [(1, 1, 1), (1, 1, 5), (3, 1, 2), (2, 3, 4), (5, 4, 3), (8, 8, 8), (4, 8, 7)]


def random_mask(rng, shape, p):
    return rng.random(shape) < p


def surface_brute(mask, element):
    most = {6: 1, 18: 2, 26: 3}[element]
    nz, ny, nx = mask.shape
    out = np.zeros_like(mask)
    for z, y, x in np.argwhere(mask):
        for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3):
            if not 0 < (dz != 0) + (dy != 0) + (dx != 0) <= most:
                continue
            q = (z + dz, y + dy, x + dx)
            if not (0 <= q[0] < nz and 0 <= q[1] < ny and 0 <= q[2] < nx) or not mask[q]:
                out[z, y, x] = True
    return out


@pytest.mark.parametrize("shape", TINY)
@pytest.mark.parametrize("element", [6, 18, 26])
def test_reference_surface_is_the_definition(shape, element):
    rng = np.random.default_rng(hash((shape, element)) & 0xFFFF)
    for p in (0.0, 0.3, 0.8, 1.0):
        m = random_mask(rng, shape, p)
        assert np.array_equal(cr.surface(m, element), surface_brute(m, element))


def test_reference_surface_of_full_and_box():
    full = np.ones((5, 6, 7), bool)
    faces = np.ones_like(full)
    faces[1:-1, 1:-1, 1:-1] = False
    for element in (6, 18, 26):
        assert np.array_equal(cr.surface(full, element), faces)
    box = np.zeros((7, 8, 9), bool)
    box[1:6, 2:7, 1:8] = True
    shell = box.copy()
    shell[2:5, 3:6, 2:7] = False
    assert np.array_equal(cr.surface(box, 26), shell)


@pytest.mark.parametrize("shape", TINY)
@pytest.mark.parametrize("weights", [(1, 1, 1), (1, 4, 9)])
def test_reference_compare_is_brute_force(shape, weights):
    rng = np.random.default_rng(hash((shape, weights)) & 0xFFFF)
    for pa, pb in ((0.5, 0.5), (0.9, 0.2), (0.3, 0.0), (0.0, 0.0)):
        a, b = random_mask(rng, shape, pa), random_mask(rng, shape, pb)
        tol = (0, 1, 4)
        c = cr.compare(a, b, 18, weights, (90, 100), tol)
        assert c["overlap"] == [int((a & b).sum()), int((a & ~b).sum()), int((~a & b).sum()), int((~a & ~b).sum())]
        assert c["status"] == (0 if a.any() else cr.A_EMPTY) | (0 if b.any() else cr.B_EMPTY)
        sa, sb = surface_brute(a, 18), surface_brute(b, 18)
        assert c["surface"] == [int(sa.sum()), int(sb.sum())]
        for name, src, dst in (("ab", sa, sb), ("ba", sb, sa)):
            d = cr.directed_brute(src, dst, weights)
            s = c[name]
            if d is None:
                assert (s["voxels"], s["none"], s["sum"], s["max"], c["quantile_" + name]) == (0, int(src.sum()), 0, 0, 0)
                continue
            assert (s["voxels"], s["none"], s["sum"]) == (len(d), 0, sum(d))
            assert s["sum_root_q8"] == sum(math.isqrt(t << 16) for t in d)
            assert s["max"] == max(d, default=0)
            idx = np.flatnonzero(src.reshape(-1))
            assert s["first_max"] == (int(idx[d.index(max(d))]) if d else 0)
            assert s["within"][:3] == [sum(1 for t in d if t <= k) for k in tol]
            if d:                                             # inverted_cdf: the ceil(q n)-th smallest value
                assert c["quantile_" + name] == sorted(d)[max(-(-90 * len(d) // 100), 1) - 1]


def test_reference_quantile_and_histogram():
    rng = np.random.default_rng(5)
    d2 = rng.integers(0, 50, (3, 4, 5)).astype(np.uint32)
    d2[0, 0, :3] = cr.NONE
    m = rng.random(d2.shape) < 0.6
    vals = np.sort(d2[m & (d2 != cr.NONE)])
    for num, den in ((0, 1), (1, 2), (95, 100), (1, 1)):
        assert cr.quantile(d2, num, den, m) == int(vals[max(-(-num * len(vals) // den), 1) - 1])
    h = cr.histogram(d2, m, 3, 40, 2)
    assert len(h) == 10 and int(h.sum()) == int(((vals >= 3) & (vals <= 40)).sum())
    assert int(cr.histogram(d2, None, 0, cr.NONE, 31)[1]) == int((d2 >= 1 << 31).sum()) == 3
    assert cr.quantile(np.full((1, 1, 2), cr.NONE, np.uint32), 1, 2) is None


# ---------------- the library's host code ----------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    return lib


def test_struct_sizes_are_the_header_comments():
    assert (C.sizeof(abi.DistanceSummary), C.sizeof(abi.CompareParams), C.sizeof(abi.RegionComparison), C.sizeof(abi.CompareMeasurement)) == (72, 60, 208, 152)
    assert abi.RegionComparison.ab.offset == 48 and abi.RegionComparison.ba.offset == 120 and abi.RegionComparison.quantile_ab.offset == 192


def test_compare_params_default(lib):
    p = host.compare_params(lib=lib)
    assert (p.element, list(p.weights), p.q_num, p.q_den, p.ntol, list(p.tolerances2)) == (6, [1, 1, 1], 95, 100, 0, [0] * 8)


def test_overlap_match_against_fractions(lib):
    rng = np.random.default_rng(11)
    for ca, cb in ((1, 1), (3, 5), (6, 2), (9, 9)):
        for density in (0.2, 0.7):
            t = (rng.integers(0, 40, (ca + 1, cb + 1)) * (rng.random((ca + 1, cb + 1)) < density)).astype(np.uint32)
            best_b, best_a = host.overlap_match(t, lib)
            ref_b, ref_a = cr.overlap_match(t)
            assert list(best_b) == ref_b and list(best_a) == ref_a


def test_overlap_match_ties_background_and_large_counts(lib):
    # label 1 of A meets 1 and 2 of B with the same index 2 / (4 + 2 - 2): the lower label wins; label 2 of A meets only the background
    t = np.array([[0, 0, 0, 5], [0, 2, 2, 0], [7, 0, 0, 0]], dtype=np.uint32)
    best_b, best_a = host.overlap_match(t, lib)
    assert list(best_b) == [1, 0] and list(best_a) == [1, 1, 0]
    assert (list(best_b), list(best_a)) == tuple(cr.overlap_match(t))
    # the background cells count in the sizes: B's label 2 is mostly background of A, so A's label 1 prefers B's label 1 (3 / 5 > 4 / 13)
    t = np.array([[0, 0, 9], [2, 3, 4]], dtype=np.uint32)
    assert list(host.overlap_match(t, lib)[0]) == [1] == cr.overlap_match(t)[0]
    # cross products beyond 64 bits: cells near 2^32
    big = np.array([[0, 1, 0], [0, 0xFFFFFFFF, 0xFFFFFFFE], [0, 0xFFFFFFFE, 0xFFFFFFFF]], dtype=np.uint32)
    best_b, best_a = host.overlap_match(big, lib)
    assert (list(best_b), list(best_a)) == tuple(cr.overlap_match(big)) == ([1, 2], [1, 2])


def example_comparison():
    rng = np.random.default_rng(3)
    a, b = rng.random((6, 7, 8)) < 0.5, rng.random((6, 7, 8)) < 0.4
    return cr.compare(a, b, 6, (1, 1, 4), (95, 100), (0, 1, 2, 9))


def close(x, y):
    if isinstance(y, list):
        return all(close(s, t) for s, t in zip(x, y)) and len(x) == len(y)
    if math.isnan(y):
        return math.isnan(x)
    return abs(x - y) <= 1e-12 * abs(y)                        # the same float64 expression: a handful of roundings of 2^-53


def measured(lib, c, unit):
    m = host.compare_measure(cr.struct_of_comparison(c), unit, lib)
    return {name: (list(getattr(m, name)) if name == "surface_dice" else float(getattr(m, name))) for name, _ in abi.CompareMeasurement._fields_}


@pytest.mark.parametrize("unit", [1.0, 0.3125])
def test_compare_measure_is_the_formulas(lib, unit):
    c = example_comparison()
    assert c["ab"]["voxels"] and c["ba"]["voxels"] and c["ntol"] == 4
    got, want = measured(lib, c, unit), cr.measure(c, unit)
    assert set(got) == set(want)
    for name in want:
        assert close(got[name], want[name]), (name, got[name], want[name])
    assert 0.0 < got["dice"] < 1.0 and got["hausdorff"] >= got["hausdorff_q"] >= 0.0 and got["rms"] >= got["assd"] > 0.0


def test_compare_measure_nan_cases(lib):
    e, f = np.zeros((3, 3, 3), bool), np.ones((3, 3, 3), bool)
    both_empty = measured(lib, cr.compare(e, e), 1.0)
    for name in ("dice", "jaccard", "volume_difference", "hausdorff_ab", "hausdorff_ba", "hausdorff", "hausdorff_q", "assd", "rms"):
        assert math.isnan(both_empty[name]), name
    assert both_empty["surface_dice"] == [0.0] * 8            # ntol = 0: none is computed
    c = cr.compare(f, e, tolerances2=(1,))
    assert c["status"] == cr.B_EMPTY and c["ab"]["none"] == 26 and c["ab"]["voxels"] == 0
    one_empty = measured(lib, c, 1.0)
    assert (one_empty["dice"], one_empty["jaccard"], one_empty["volume_difference"]) == (0.0, 0.0, 2.0)
    for name in ("hausdorff_ab", "hausdorff_ba", "hausdorff", "hausdorff_q_ab", "hausdorff_q", "assd", "rms"):
        assert math.isnan(one_empty[name]), name
    assert one_empty["surface_dice"][0] == 0.0                # 0 of 26 surface voxels lie within the tolerance
    for got, want in ((both_empty, cr.measure(cr.compare(e, e))), (one_empty, cr.measure(c))):
        assert all(close(got[name], want[name]) for name in want)
    same = measured(lib, cr.compare(f, f, tolerances2=(0,)), 2.0)
    assert (same["dice"], same["jaccard"], same["volume_difference"], same["hausdorff"], same["assd"], same["rms"], same["surface_dice"][0]) == \
        (1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)


# ---------------- the refusals, before the device is touched ----------------
def refuse(lib, name, *args):
    lib.svr_clear_error()
    rc = getattr(lib, name)(*args)
    text = lib.svr_last_error().decode()
    assert lib.svr_last_error_code() == rc
    lib.svr_clear_error()
    return rc, text


class Buffers:
    """64-byte host buffers standing in for device memory: the refused calls never read them"""

    def __init__(self):
        self.keep = []

    def __call__(self, nbytes=64):
        self.keep.append(np.zeros(nbytes, np.uint8))
        return C.c_void_p(self.keep[-1].ctypes.data)


def u32s(*v):
    return (C.c_uint32 * len(v))(*v)


def dims(*v):
    return (C.c_int32 * 3)(*v)


def refusal_cases():
    """(id, function, arguments, code, a word of the message)"""
    buf = Buffers()
    a, b, out, big = buf(), buf(), buf(), buf(4096)
    inside = C.c_void_p(big.value + 64)
    counts, summ, comp = (C.c_uint64 * 4)(), abi.DistanceSummary(), abi.RegionComparison()
    value, status = C.c_uint32(0), C.c_int32(0)
    good, bad_dims = (4, 4, 4), [(0, 4, 4), (4, -1, 4), (4, 4, 0), (2048, 2048, 1024)]

    def params(**kw):
        p = abi.CompareParams(6, u32s(1, 1, 1), 95, 100, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)
    cases = []

    def add(rid, name, args, code, word):
        cases.append(pytest.param(name, args, code, word, id=f"{name[4:]}/{rid}"))
    # null pointers
    add("null in", "svr_region_surface", (None, *good, 6, out), -4, "null")
    add("null out", "svr_region_surface", (a, *good, 6, None), -4, "null")
    add("null b", "svr_region_overlap", (a, None, *good, None, counts), -4, "null")
    add("null counts", "svr_region_overlap", (a, b, *good, None, None), -4, "null")
    add("null b", "svr_region_label_overlap", (a, 2, None, 2, dims(*good), out), -4, "null")
    add("null dims", "svr_region_label_overlap", (a, 2, b, 2, None, out), -4, "null")
    add("null table", "svr_overlap_match", (None, 2, 2, u32s(0, 0), None), -4, "null")
    add("null best", "svr_overlap_match", (a, 2, 2, None, None), -4, "null")
    add("null map", "svr_region_distance_summary", (None, None, *good, None, 0, C.byref(summ)), -4, "null")
    add("null out", "svr_region_distance_summary", (a, None, *good, None, 0, None), -4, "null")
    add("null tolerances", "svr_region_distance_summary", (a, None, *good, None, 2, C.byref(summ)), -4, "null")
    add("null counts", "svr_region_distance_histogram", (a, None, dims(*good), 0, 9, 0, None), -4, "null")
    add("null value", "svr_region_distance_quantile", (a, None, dims(*good), 1, 2, None, C.byref(status)), -4, "null")
    add("null status", "svr_region_distance_quantile", (a, None, dims(*good), 1, 2, C.byref(value), None), -4, "null")
    add("null", "svr_compare_params_default", (None,), -4, "null")
    add("null a", "svr_region_compare", (None, b, *good, None, C.byref(comp)), -4, "null")
    add("null out", "svr_region_compare", (a, b, *good, None, None), -4, "null")
    add("null c", "svr_region_compare_measure", (None, 1.0, C.byref(abi.CompareMeasurement())), -4, "null")
    add("null out", "svr_region_compare_measure", (C.byref(comp), 1.0, None), -4, "null")
    add("null", "svr_region_compare_last_ms", (None,), -4, "null")
    # dimensions
    for d in bad_dims:
        word = "2^31" if d[0] == 2048 else "bad dimensions"
        add(f"dims {d}", "svr_region_surface", (a, *d, 6, out), -6, word)
        add(f"dims {d}", "svr_region_overlap", (a, b, *d, None, counts), -6, word)
        add(f"dims {d}", "svr_region_label_overlap", (a, 2, b, 2, dims(*d), out), -6, word)
        add(f"dims {d}", "svr_region_distance_summary", (a, None, *d, None, 0, C.byref(summ)), -6, word)
        add(f"dims {d}", "svr_region_distance_histogram", (a, None, dims(*d), 0, 9, 0, out), -6, word)
        add(f"dims {d}", "svr_region_distance_quantile", (a, None, dims(*d), 1, 2, C.byref(value), C.byref(status)), -6, word)
        add(f"dims {d}", "svr_region_compare", (a, b, *d, None, C.byref(comp)), -6, word)
    # the rest
    for element in (0, 7, 27):
        add(f"element {element}", "svr_region_surface", (a, *good, element, out), -3, "element must be 6, 18 or 26")
        add(f"element {element}", "svr_region_compare", (a, b, *good, params(element=element), C.byref(comp)), -3, "element must be 6, 18 or 26")
    add("out is in", "svr_region_surface", (a, *good, 6, a), -3, "overlap")
    add("out inside in", "svr_region_surface", (big, 64, 4, 4, 6, inside), -3, "overlap")
    add("weight 0", "svr_region_compare", (a, b, *good, params(weights=u32s(1, 0, 1)), C.byref(comp)), -3, "weight")
    add("overflow bound", "svr_region_compare", (a, b, 300, 300, 3, params(weights=u32s(30000, 30000, 1)), C.byref(comp)), -3, "overflow")
    add("ntol 9", "svr_region_compare", (a, b, *good, params(ntol=9), C.byref(comp)), -3, "ntol")
    add("den 0", "svr_region_compare", (a, b, *good, params(q_den=0), C.byref(comp)), -3, "quantile")
    add("num > den", "svr_region_compare", (a, b, *good, params(q_num=101), C.byref(comp)), -3, "quantile")
    add("ntol 9", "svr_region_distance_summary", (a, None, *good, u32s(*range(9)), 9, C.byref(summ)), -3, "ntol")
    add("lo > hi", "svr_region_distance_histogram", (a, None, dims(*good), 10, 9, 0, out), -3, "above hi")
    add("65537 bins", "svr_region_distance_histogram", (a, None, dims(*good), 0, 65536, 0, out), -3, "bins")
    add("65537 bins shifted", "svr_region_distance_histogram", (a, None, dims(*good), 0, 0xFFFFFFFF, 15, out), -3, "bins")
    add("shift 32", "svr_region_distance_histogram", (a, None, dims(*good), 0, 9, 32, out), -3, "shift")
    add("counts inside map", "svr_region_distance_histogram", (big, None, dims(8, 8, 8), 0, 9, 0, inside), -3, "overlap")
    add("counts is mask", "svr_region_distance_histogram", (big, a, dims(*good), 0, 9, 0, a), -3, "overlap")
    add("den 0", "svr_region_distance_quantile", (a, None, dims(*good), 0, 0, C.byref(value), C.byref(status)), -3, "quantile")
    add("num > den", "svr_region_distance_quantile", (a, None, dims(*good), 3, 2, C.byref(value), C.byref(status)), -3, "quantile")
    add("count_a 0", "svr_region_label_overlap", (a, 0, b, 2, dims(*good), out), -3, "at least 1")
    add("count_b 0", "svr_region_label_overlap", (a, 2, b, 0, dims(*good), out), -3, "at least 1")
    add("too many cells", "svr_region_label_overlap", (a, 4095, b, 4096, dims(*good), out), -3, "SVR_HISTOGRAM_MAX_CELLS")
    add("table inside labels", "svr_region_label_overlap", (big, 2, b, 2, dims(8, 8, 8), inside), -3, "overlap")
    add("table is b", "svr_region_label_overlap", (a, 1, big, 1, dims(8, 8, 8), big), -3, "overlap")
    add("count_a 0", "svr_overlap_match", (a, 0, 2, u32s(0, 0), None), -3, "at least 1")
    add("count_b 0", "svr_overlap_match", (a, 2, 0, u32s(0, 0), None), -3, "at least 1")
    add("ntol 9", "svr_region_compare_measure", (C.byref(abi.RegionComparison(ntol=9)), 1.0, C.byref(abi.CompareMeasurement())), -3, "ntol")
    cases.append(buf)                                         # (keeps the buffers alive)
    return cases


_CASES = refusal_cases()


@pytest.mark.parametrize("name,args,code,word", _CASES[:-1])
def test_refusals(lib, name, args, code, word):
    rc, text = refuse(lib, name, *args)
    assert rc == code and name in text and word in text, (rc, text)


def test_the_largest_table_is_not_refused_for_its_size(lib):
    """4095 x 4095 labels are exactly SVR_HISTOGRAM_MAX_CELLS cells: the call gets past that check (to the overlap check, here)"""
    buf = Buffers()
    a = buf()
    rc, text = refuse(lib, "svr_region_label_overlap", a, 4095, a, 4095, dims(4, 4, 4), a)
    assert rc == -3 and "overlap" in text


# ---------------- the Python methods on the fake device ----------------
S = (2, 3, 33)
_rng = np.random.default_rng(77)
M, M2, DOM = _rng.random(S) < 0.5, _rng.random(S) < 0.3, _rng.random(S) < 0.8
LAB, LAB2 = _rng.integers(0, 4, S).astype(np.uint32), _rng.integers(0, 6, S).astype(np.uint32)
D2 = _rng.integers(0, 100, S).astype(np.uint32)
W = host.region_mask_words(S)


def R(rid, name, *args, **kwargs):
    return (rid, name, args, kwargs)


ROWS = [
    R("region_surface/host", "region_surface", M, 18),
    R("region_surface/dev", "region_surface", Dev(M), shape=S, out_ptr=Out(4 * W)),
    R("region_overlap/host", "region_overlap", M, M2, DOM),
    R("region_overlap/dev", "region_overlap", Dev(M), Dev(M2), shape=S),
    R("region_label_overlap/host", "region_label_overlap", LAB, 3, LAB2, 5),
    R("region_label_overlap/dev", "region_label_overlap", Dev(LAB), 3, Dev(LAB2), 5, shape=S, out_ptr=Out(4 * 4 * 6)),
    R("region_distance_summary/host", "region_distance_summary", D2, M, (1, 4, 9)),
    R("region_distance_summary/dev", "region_distance_summary", Dev(D2), Dev(M), shape=S),
    R("region_distance_histogram/host", "region_distance_histogram", D2, M, 2, 90, 3),
    R("region_distance_histogram/dev", "region_distance_histogram", Dev(D2), None, 0, 99, shape=S, out_ptr=Out(400)),
    R("region_distance_quantile/host", "region_distance_quantile", D2, 95, 100, M),
    R("region_distance_quantile/dev", "region_distance_quantile", Dev(D2), 1, 2, Dev(M), shape=S),
    R("region_compare/host", "region_compare", M, M2, 26, (1, 1, 4), (90, 100), (1, 2)),
    R("region_compare/dev", "region_compare", Dev(M), Dev(M2), shape=S),
    R("region_compare_last_ms", "region_compare_last_ms"),
]
IDS = [row[0] for row in ROWS]
CALLS = {"region_surface": ["svr_region_surface"], "region_overlap": ["svr_region_overlap"], "region_label_overlap": ["svr_region_label_overlap"],
         "region_distance_summary": ["svr_region_distance_summary"], "region_distance_histogram": ["svr_region_distance_histogram"],
         "region_distance_quantile": ["svr_region_distance_quantile"], "region_compare": ["svr_compare_params_default", "svr_region_compare"],
         "region_compare_last_ms": ["svr_region_compare_last_ms"]}


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_fake_device_calls_and_no_leak(row):
    dev, caller, result = run_row(row)
    assert not isinstance(result, Exception), result
    assert [c["fn"] for c in dev.lib.calls] == CALLS[row[1]]
    assert dev.live == set(caller)
    call = dev.lib.calls[-1]["args"]
    if row[1] not in ("region_compare_last_ms",):
        assert call[0][0] == "dev"                            # the first operand reached the library as device memory
    if row[0].endswith("/dev") and row[1] == "region_surface":
        assert call[-1][:2] == ["dev", 4 * W]                 # the caller's buffer is the output


def test_fake_device_arguments():
    dev, _, _ = run_row(R("x", "region_compare", M, M2, 26, (1, 1, 4), (90, 100), (1, 2)))
    args = dev.lib.calls[-1]["args"]
    assert args[2:5] == [33, 3, 2]
    assert args[5] == {"element": 26, "weights": [1, 1, 4], "q_num": 90, "q_den": 100, "ntol": 2, "tolerances2": [1, 2, 0, 0, 0, 0, 0, 0]}
    dev, _, _ = run_row(R("x", "region_distance_histogram", D2, M, 2, 90, 3))
    args = dev.lib.calls[-1]["args"]
    assert args[2:6] == [[33, 3, 2], 2, 90, 3] and args[6][:2] == ["dev", 4 * 12]
    dev, _, _ = run_row(R("x", "region_label_overlap", LAB, 3, LAB2, 5))
    args = dev.lib.calls[-1]["args"]
    assert (args[1], args[3], args[4]) == (3, 5, [33, 3, 2]) and args[5][:2] == ["dev", 4 * 24]
    dev, _, _ = run_row(R("x", "region_distance_summary", D2, None, (1, 4, 9)))
    args = dev.lib.calls[-1]["args"]
    assert args[1] is None and args[5:7] == [[1, 4, 9], 3]


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_fake_device_no_leak_on_failure(row):
    dev, caller, _ = run_row(row)
    mallocs, calls = dev.nmalloc, dev.lib.ncalls
    assert calls >= 1
    for k in range(1, mallocs + 1):
        dev, caller, result = run_row(row, fail_malloc=k)
        assert isinstance(result, SvrError) and "injected malloc failure" in str(result), (k, result)
        assert dev.live == set(caller), f"malloc {k} of {mallocs} failed"
    for k in range(1, calls + 1):
        dev, caller, result = run_row(row, fail_call=k)
        assert isinstance(result, SvrError) and "injected failure of svr_" in str(result), (k, result)
        assert dev.live == set(caller), f"library call {k} of {calls} failed"


def test_fake_device_shape_errors_leave_nothing():
    for row, message in ((R("x", "region_label_overlap", LAB, 3, LAB2.reshape(3, 2, 33), 5), "differ in shape"),
                         (R("x", "region_overlap", M, M2[:1]), "reshape"),
                         (R("x", "region_surface", 1 << 60), "a device mask needs shape")):
        dev, caller, result = run_row(row)
        assert isinstance(result, ValueError) and message in str(result), result
        assert dev.live == set(caller)
