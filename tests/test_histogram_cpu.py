"""The host side of the histogram calls (include/svr_abi.h, "histograms of the u16 voxels"): svr_histogram_moments /
_quantile / _otsu / _bins / _bin_range against the exact reference of tests/histogram_ref.py, the reference itself against numpy's
inverted_cdf percentile and a textbook float Otsu, and every refusal of the two device calls, which stands before the device is touched
so the library answers without a GPU."""
import ctypes as C
import random

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import histogram_ref as hr


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    lib.svr_clear_error()
    return lib


@pytest.fixture(scope="module")
def head():
    return scenes.make_ct_head_volume(48)


def c_otsu(lib, counts, classes):
    return host.histogram_otsu(counts, classes, lib)


def sparse(bins, pos, cnt):
    h = np.zeros(bins, np.uint32)
    h[list(pos)] = cnt
    return h


# ---- the reference against independent formulations ----
def test_reference_quantile_is_numpys_inverted_cdf():
    rng = np.random.default_rng(5)
    for n, top in ((1, 5), (7, 3), (100, 40), (1001, 256), (4096, 9)):
        data = rng.integers(0, top, n)
        counts = np.bincount(data, minlength=top)
        for num, den in ((1, 1000), (1, 4), (1, 2), (2, 3), (99, 100), (999, 1000), (1, 1), (1, n), (n - 1 or 1, n)):
            want = int(np.percentile(data, 100.0 * num / den, method="inverted_cdf"))
            # (the float percent of numpy can round num / den * n across an integer: compare where q n is safely off one)
            if abs(num * n / den - round(num * n / den)) < 1e-9 and num * n % den != 0:
                continue
            assert hr.quantile(counts, num, den) == want, (n, top, num, den)
        assert hr.quantile(counts, 0, 1) == int(data.min()) and hr.quantile(counts, 1, 1) == int(data.max())


def test_reference_two_class_otsu_is_the_float_otsu_on_clear_maxima():
    rng = np.random.default_rng(6)
    for bins in (2, 3, 16, 200):
        for _ in range(6):
            a, b = sorted(rng.choice(bins, 2, replace=False)) if bins > 2 else (0, 1)
            counts = rng.integers(0, 5, bins)
            counts[a] += 1000
            counts[b] += 700                                               # two modes: one clear maximum, far from any tie
            assert hr.otsu(counts, 2)[0][0] == hr.otsu2_float(counts) == hr.otsu2_fast(counts), counts


# ---- the C analysis against the reference ----
def check_all(lib, counts, classes=(2, 3)):
    counts = np.asarray(counts, np.uint32)
    assert host.histogram_moments(counts, lib) == hr.moments(counts)
    for num, den in ((0, 1), (1, 1000), (1, 2), (1, 3), (999, 1000), (1, 1), (7, 7)):
        assert host.histogram_quantile(counts, num, den, lib) == hr.quantile(counts, num, den), (num, den)
    got = {}
    for k in classes:
        if len(counts) < k or (k == 3 and len(counts) > 256):
            continue
        want_t, want_eta = hr.otsu(counts, k)
        t, eta = c_otsu(lib, counts, k)
        assert t == want_t, (k, t, want_t)
        assert eta == pytest.approx(want_eta, rel=1e-9, abs=1e-12) and 0.0 <= eta <= 1.0
        got[k] = t
    return got


def test_c_analysis_matches_the_reference_on_random_histograms(lib):
    rng = np.random.default_rng(7)
    for bins in (1, 2, 3, 4, 5, 17, 64, 256):
        for hi in (2, 10, 1000, 1 << 20):
            check_all(lib, rng.integers(0, hi, bins))
        h = rng.integers(0, 100, bins)
        h[rng.random(bins) < 0.7] = 0                                      # mostly empty bins: empty classes and ties
        check_all(lib, h)
    for bins in (300, 1000):                                               # two classes only
        check_all(lib, rng.integers(0, 1 << 16, bins), classes=(2,))


def test_c_analysis_on_the_head(lib, head):
    h0 = hr.histogram(head)
    assert int(h0[0]) * 1000 // head.size == 676 and int((h0 > 0).sum()) == 18252          # 67.6 % zeros, 18 252 occupied bins
    t0 = c_otsu(lib, h0, 2)[0]
    assert t0 == (hr.otsu2_fast(h0),)
    assert host.histogram_moments(h0, lib) == hr.moments(h0)
    for num, den in ((0, 1), (1, 2), (7, 10), (99, 100), (1, 1)):
        assert host.histogram_quantile(h0, num, den, lib) == hr.quantile(h0, num, den)
    h8 = hr.histogram(head, shift=8)
    got = check_all(lib, h8)
    print(f"head 48^3: two-class Otsu bin {t0[0]} at shift 0, {got[2][0]} at shift 8; three-class at shift 8 {got[3]}")
    assert t0 == (15649,) and got[2] == (60,) and got[3] == (51, 132)


def test_c_analysis_on_degenerate_histograms(lib):
    for bins in (2, 3, 9, 256):
        for at in sorted({0, bins // 2, bins - 1}):
            got = check_all(lib, sparse(bins, [at], [5]))                  # a single occupied bin: every tuple ties, the smallest wins
            assert got[2] == (0,) and (bins < 3 or got[3] == (0, 1))
    got = check_all(lib, sparse(10, [2, 7], [3, 4]))                       # two occupied bins: the cut is at the first, every t in 2 .. 6 ties
    assert got[2] == (2,) and got[3] == (0, 2)
    assert check_all(lib, sparse(256, [0, 255], [1, 1]))[2] == (0,)
    assert host.histogram_moments(sparse(1, [0], [9]), lib) == (9, 0, 0)
    assert host.histogram_quantile(sparse(1, [0], [9]), 1, 2, lib) == 0


def test_c_analysis_with_the_largest_counts(lib):
    # 2^31 in one bin (a whole volume of one value), 0xFFFFFFFF in several (a caller's own counts): N up to 2^37 and more
    full = 0xFFFFFFFF
    for counts in (sparse(65536, [65535], [1 << 31]), sparse(65536, [0, 1, 65535], [1 << 31, 1, 1]),
                   sparse(4096, [1, 100, 4095], [full, full, full]), np.full(200, full, np.uint32)):
        assert host.histogram_moments(counts, lib) == hr.moments(counts)
        for num, den in ((0, 1), (1, 3), (1, 2), (2, 3), (full - 1, full), (full, full), (1, full)):
            assert host.histogram_quantile(counts, num, den, lib) == hr.quantile(counts, num, den), (num, den)
        assert c_otsu(lib, counts, 2)[0] == (hr.otsu2_fast(counts),)
    # N = 2^48: the quantile still compares exactly (den * C(b) needs 80 bits); the second moment no longer fits and is refused
    counts = np.full(65536, full, np.uint32)
    for num, den in ((1, 2), (32768, 65536), (32769, 65536), (full - 1, full)):
        assert host.histogram_quantile(counts, num, den, lib) == hr.quantile(counts, num, den)
    with pytest.raises(host.SvrError, match="64 bits"):
        host.histogram_moments(counts, lib)
    check_all(lib, np.full(256, full, np.uint32))                          # three classes at the largest counts


def test_empty_histogram_is_a_status_not_an_error(lib):
    for bins in (1, 2, 256, 65536):
        z = np.zeros(bins, np.uint32)
        p = z.ctypes.data_as(C.c_void_p)
        n, s, q, b, eta = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7), C.c_uint32(7), C.c_double(7.0)
        t = (C.c_uint32 * 2)(7, 7)
        lib.svr_clear_error()
        assert lib.svr_histogram_moments(p, bins, C.byref(n), C.byref(s), C.byref(q)) == abi.HISTOGRAM_STATUS_EMPTY
        assert (n.value, s.value, q.value) == (0, 0, 0)
        assert lib.svr_histogram_quantile(p, bins, 1, 2, C.byref(b)) == abi.HISTOGRAM_STATUS_EMPTY and b.value == 0
        if bins >= 2:
            assert lib.svr_histogram_otsu(p, bins, 2, t, C.byref(eta)) == abi.HISTOGRAM_STATUS_EMPTY and (t[0], eta.value) == (0, 0.0)
        if 3 <= bins <= 256:
            t[0] = 7
            assert lib.svr_histogram_otsu(p, bins, 3, t, None) == abi.HISTOGRAM_STATUS_EMPTY and (t[0], t[1]) == (0, 0)
        assert lib.svr_last_error_code() == 0
        assert host.histogram_quantile(z, 1, 2, lib) is None and host.histogram_otsu(z, 2, lib) == (None, 0.0) if bins >= 2 else True


def test_exact_ties_go_to_the_lower_threshold(lib):
    # a symmetric histogram: the cuts t and bins - 2 - t give mirrored classes and exactly the same criterion
    for counts in ([5, 1, 5], [9, 2, 0, 2, 9], [7, 3, 1, 1, 3, 7], [1 << 30, 12345, 99, 12345, 1 << 30], [4, 0, 0, 4], [1, 1, 1, 1, 1, 1, 1]):
        t = c_otsu(lib, counts, 2)[0][0]
        mirrored = len(counts) - 2 - t
        assert hr.otsu_criterion(counts, (t,)) == hr.otsu_criterion(counts, (mirrored,)) and t <= mirrored
        assert (t,) == hr.otsu(counts, 2)[0]
        if len(counts) >= 3:
            assert c_otsu(lib, counts, 3)[0] == hr.otsu(counts, 3)[0]
    assert c_otsu(lib, [5, 1, 5], 2)[0] == (0,) and c_otsu(lib, [4, 0, 0, 4], 2)[0] == (0,)
    # three classes on a symmetric histogram with several maximisers: (0, 2) and (1, 3) tie
    counts = [6, 0, 6, 0, 6]
    assert hr.otsu_criterion(counts, (0, 2)) == hr.otsu_criterion(counts, (1, 3)) == hr.otsu_criterion(counts, (1, 2))
    assert c_otsu(lib, counts, 3)[0] == (0, 2) == hr.otsu(counts, 3)[0]


def float64_otsu(pos, cnt):
    """the criterion S1^2 / N1 + S2^2 / N2 evaluated in float64 at the occupied bins (between them it does not change), first maximum"""
    c, p = np.array(cnt, np.float64), np.array(pos, np.float64)
    n1, s1 = np.cumsum(c)[:-1], np.cumsum(c * p)[:-1]
    n2, s2 = c.sum() - n1, (c * p).sum() - s1
    return pos[int(np.argmax(s1 * s1 / n1 + s2 * s2 / n2))]


def float64_fraction_otsu(pos, cnt):
    """the same criterion as ONE fraction (S1^2 N2 + S2^2 N1) / (N1 N2) whose exact numerator and denominator are each rounded to float64
    and then divided, first maximum: the evaluation with the fewest roundings a double comparison can have"""
    best, best_at = -1.0, 0
    for k in range(len(pos) - 1):
        n1, s1 = sum(cnt[:k + 1]), sum(a * b for a, b in zip(pos[:k + 1], cnt[:k + 1]))
        n2, s2 = sum(cnt[k + 1:]), sum(a * b for a, b in zip(pos[k + 1:], cnt[k + 1:]))
        value = float(s1 * s1 * n2 + s2 * s2 * n1) / float(n1 * n2)
        if value > best:
            best, best_at = value, pos[k]
    return best_at


def sparse_criterion(pos, cnt, k):
    """the criterion of the cut after the k-th occupied bin, as a Fraction"""
    from fractions import Fraction
    p, c = [int(t) for t in pos], [int(t) for t in cnt]
    n1, s1 = sum(c[:k + 1]), sum(a * b for a, b in zip(p[:k + 1], c[:k + 1]))
    n2, s2 = sum(c[k + 1:]), sum(a * b for a, b in zip(p[k + 1:], c[k + 1:]))
    return Fraction(s1 * s1, n1) + Fraction(s2 * s2, n2)


def near_ties(want=4, tries=4000):
    """Histograms on which float64 picks another threshold than exact arithmetic: five groups, symmetric about the middle bin of 65535
    bins with totals near 2^30, so the cuts after the second and after the third group tie exactly; then one count is moved by one (or
    none: the rounding of the two mirrored evaluations differs by itself).  Found by search, so the case cannot silently stop testing."""
    rng = random.Random(1)
    found = []
    for _ in range(tries):
        a = rng.randrange(1, 15000)
        b = rng.randrange(a + 1, 30000)
        pos = [a, b, 32767, 65534 - b, 65534 - a]
        big_a, big_b, mid = rng.randrange(1 << 27, 1 << 28), rng.randrange(1 << 27, 1 << 28), rng.randrange(1, 1000)
        cnt = [big_a, big_b, mid, big_b, big_a]
        k = rng.randrange(6)
        if k < 5:
            cnt[k] += 1
        counts = sparse(65535, pos, cnt)
        exact = hr.otsu2_fast(counts)
        if float64_otsu(pos, cnt) != exact and float64_fraction_otsu(pos, cnt) != exact:      # both float evaluations go wrong
            found.append((counts, exact, float64_otsu(pos, cnt)))
            if len(found) == want:
                break
    return found


def test_otsu_is_exact_where_float64_picks_another_threshold(lib):
    cases = near_ties()
    assert len(cases) == 4, "the search no longer finds histograms on which float64 disagrees"
    for counts, exact, in_float in cases:
        assert in_float != exact                                           # the float evaluation does disagree on this histogram
        assert c_otsu(lib, counts, 2)[0] == (exact,)
        # the Fraction brute force on the occupied bins alone says the same as the one-pass reference
        support = np.flatnonzero(counts)
        best = max(range(len(support) - 1), key=lambda k: (sparse_criterion(support, counts[support], k), -k))
        assert int(support[best]) == exact


# ---- bins and bin ranges ----
def test_bins_and_bin_range(lib):
    for lo, hi, shift in ((0, 65535, 0), (0, 65535, 8), (0, 65535, 15), (100, 1100, 3), (100, 1099, 3), (5, 5, 0), (5, 5, 15), (0, 65535, 3),
                          (1, 65535, 15), (32768, 65535, 15), (0, 32768, 15), (17, 60000, 7)):
        n = host.histogram_bins(lo, hi, shift, lib)
        assert n == hr.bins(lo, hi, shift)
        covered = lo
        for b in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
            assert host.histogram_bin_range(b, lo, hi, shift, lib) == hr.bin_range(b, lo, hi, shift)
        for b in range(min(n, 40)):                                        # the ranges tile lo .. hi without a gap
            first, last = host.histogram_bin_range(b, lo, hi, shift, lib)
            assert first == covered and first <= last <= hi
            covered = last + 1
        assert host.histogram_bin_range(n - 1, lo, hi, shift, lib)[1] == hi
        with pytest.raises(host.SvrError):
            host.histogram_bin_range(n, lo, hi, shift, lib)
    assert host.histogram_bin_range(125, 100, 1100, 3, lib) == (1100, 1100)          # a partial last bin: 1001 values, 126 bins
    assert host.histogram_bins(0, 65535, 15, lib) == 2 and host.histogram_bins(5, 5, 0, lib) == 1
    for lo, hi, shift in ((6, 5, 0), (0, 65536, 0), (0, 10, 16)):
        assert host.histogram_bins(lo, hi, shift, lib) == 0                # invalid: 0, and not an error
    assert lib.svr_histogram_bins(None) == 0 and lib.svr_last_error_code() == 0


def test_pod_sizes(lib):
    assert C.sizeof(abi.HistogramParams) == 36
    p = abi.HistogramParams()
    assert lib.svr_histogram_params_default(C.byref(p)) == 0
    assert (p.lo, p.hi, p.shift, list(p.box_min), list(p.box_max)) == (0, 65535, 0, [0, 0, 0], [2**31 - 1] * 3)
    assert abi.HISTOGRAM_MAX_CELLS == 1 << 24


# ---- refusals ----
class Call:
    """One call with valid arguments in real 64-byte buffers (dims 4 x 2 x 2: 16 voxels = 32 bytes, one mask word a row); `change`
    replaces arguments by name"""

    def __init__(self, lib, name):
        self.lib, self.name = lib, name
        self.bufs = {k: np.zeros(64, np.uint8) for k in ("labels", "voxels", "mask", "counts", "params", "dims")}
        self.bufs["dims"].view(np.int32)[:3] = (4, 2, 2)
        self.params = abi.HistogramParams.from_buffer(self.bufs["params"])
        assert lib.svr_histogram_params_default(C.byref(self.params)) == 0
        self.params.shift = 12                                             # 16 bins = 64 bytes of counts
        self.count = 0

    def ptr(self, key):
        return None if self.bufs[key] is None else self.bufs[key].ctypes.data

    def run(self):
        p = {k: C.c_void_p(self.ptr(k)) if self.bufs[k] is not None else None for k in self.bufs}
        dims = C.cast(p["dims"], C.POINTER(C.c_int32)) if p["dims"] is not None else None
        params = C.cast(p["params"], C.POINTER(abi.HistogramParams)) if p["params"] is not None else None
        self.lib.svr_clear_error()
        if self.name == "svr_volume_histogram":
            rc = self.lib.svr_volume_histogram(p["voxels"], dims, 1, p["mask"], params, p["counts"])
        else:
            rc = self.lib.svr_region_label_histogram(p["labels"], p["voxels"], dims, 1, self.count, params, p["counts"])
        code, text = self.lib.svr_last_error_code(), self.lib.svr_last_error().decode()
        self.lib.svr_clear_error()
        assert code == rc and (rc == 0 or self.name in text)
        return rc, text


BOTH = ("svr_volume_histogram", "svr_region_label_histogram")


@pytest.mark.parametrize("name", BOTH)
def test_device_calls_refuse_before_the_device_is_touched(lib, name):
    required = ["voxels", "dims", "counts"] + (["labels"] if name == "svr_region_label_histogram" else [])
    for key in required:                                                   # a null pointer
        c = Call(lib, name)
        c.bufs[key] = None
        assert c.run()[0] == -4, key
    for dims in ((0, 2, 2), (4, -1, 2), (4, 2, 0), (2048, 2048, 513)):     # bad dimensions, more than 2^31 voxels
        c = Call(lib, name)
        c.bufs["dims"].view(np.int32)[:3] = dims
        assert c.run()[0] == -6, dims
    for field, value in (("lo", 65535 + 1), ("hi", 65536), ("shift", 16)):
        c = Call(lib, name)
        setattr(c.params, field, value)
        if field == "lo":
            c.params.lo, c.params.hi = 9, 8                                # lo > hi
        assert c.run()[0] == -3, field
    for bmin, bmax in (((2, 0, 0), (1, 9, 9)), ((0, 0, 0), (9, -1, 9)), ((0, 0, 2), (9, 9, 9)), ((4, 0, 0), (9, 9, 9)), ((-5, 0, 0), (-1, 9, 9))):
        c = Call(lib, name)
        c.params.box_min[:], c.params.box_max[:] = bmin, bmax              # inverted, or no voxel of the volume in it
        assert c.run()[0] == -3, (bmin, bmax)
    inputs = ["voxels"] + (["mask"] if name == "svr_volume_histogram" else ["labels"])
    for key in inputs:                                                     # counts over an input: the same buffer, and its last bytes
        for offset in (0, 28):
            c = Call(lib, name)
            c.bufs["counts"] = c.bufs[key][offset:] if offset else c.bufs[key]
            if key == "mask" and offset:
                continue                                                   # (the mask is 16 bytes: byte 28 lies past it)
            rc, text = c.run()
            assert rc == -3 and "overlap" in text, (key, offset)
    c = Call(lib, name)                                                    # -4 comes before -6 before -3
    c.bufs["counts"] = None
    c.bufs["dims"].view(np.int32)[:3] = (0, 0, 0)
    c.params.shift = 99
    assert c.run()[0] == -4
    c = Call(lib, name)
    c.bufs["dims"].view(np.int32)[:3] = (0, 0, 0)
    c.params.shift = 99
    assert c.run()[0] == -6


def test_label_histogram_refuses_more_than_the_cell_cap(lib):
    c = Call(lib, "svr_region_label_histogram")
    c.params.shift = 0                                                     # 65536 bins: 256 rows reach 2^24 cells
    c.count = 256
    rc, text = c.run()
    assert rc == -3 and "SVR_HISTOGRAM_MAX_CELLS" in text
    c.params.shift, c.count = 15, (1 << 23)                                # 2 bins, 2^23 + 1 rows
    assert c.run()[0] == -3
    c.count = 0xFFFFFFFF                                                   # (count + 1 does not wrap)
    assert c.run()[0] == -3


def test_analysis_calls_refuse(lib):
    buf = np.ones(16, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    n, s, q, b, eta = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_double(0.0)
    t = (C.c_uint32 * 16)()
    par = abi.HistogramParams()
    lib.svr_histogram_params_default(C.byref(par))
    calls = [
        (-4, lambda: lib.svr_histogram_moments(None, 16, C.byref(n), C.byref(s), C.byref(q))),
        (-4, lambda: lib.svr_histogram_moments(p, 16, None, C.byref(s), C.byref(q))),
        (-4, lambda: lib.svr_histogram_moments(p, 16, C.byref(n), None, C.byref(q))),
        (-4, lambda: lib.svr_histogram_moments(p, 16, C.byref(n), C.byref(s), None)),
        (-3, lambda: lib.svr_histogram_moments(p, 0, C.byref(n), C.byref(s), C.byref(q))),
        (-4, lambda: lib.svr_histogram_quantile(None, 16, 1, 2, C.byref(b))),
        (-4, lambda: lib.svr_histogram_quantile(p, 16, 1, 2, None)),
        (-3, lambda: lib.svr_histogram_quantile(p, 0, 1, 2, C.byref(b))),
        (-3, lambda: lib.svr_histogram_quantile(p, 16, 1, 0, C.byref(b))),
        (-3, lambda: lib.svr_histogram_quantile(p, 16, 3, 2, C.byref(b))),
        (-4, lambda: lib.svr_histogram_otsu(None, 16, 2, t, C.byref(eta))),
        (-4, lambda: lib.svr_histogram_otsu(p, 16, 2, None, C.byref(eta))),
        (-3, lambda: lib.svr_histogram_otsu(p, 0, 2, t, C.byref(eta))),
        (-3, lambda: lib.svr_histogram_otsu(p, 16, 1, t, C.byref(eta))),
        (-3, lambda: lib.svr_histogram_otsu(p, 16, 4, t, C.byref(eta))),
        (-3, lambda: lib.svr_histogram_otsu(p, 1, 2, t, C.byref(eta))),
        (-3, lambda: lib.svr_histogram_otsu(p, 2, 3, t, C.byref(eta))),
        (-3, lambda: lib.svr_histogram_otsu(np.ones(257, np.uint32).ctypes.data_as(C.c_void_p), 257, 3, t, C.byref(eta))),
        (-4, lambda: lib.svr_histogram_params_default(None)),
        (-4, lambda: lib.svr_histogram_bin_range(None, 0, C.byref(b), C.byref(b))),
        (-4, lambda: lib.svr_histogram_bin_range(C.byref(par), 0, None, C.byref(b))),
        (-3, lambda: lib.svr_histogram_bin_range(C.byref(par), 65536, C.byref(b), C.byref(b))),
        (-4, lambda: lib.svr_volume_histogram_last_ms(None)),
    ]
    for i, (want, call) in enumerate(calls):
        lib.svr_clear_error()
        rc = call()
        assert rc == want and lib.svr_last_error_code() == want, i
    lib.svr_clear_error()
