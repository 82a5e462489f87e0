"""The numpy / Python-int reference of the comparison calls (svr_region_surface, _overlap, _label_overlap, svr_overlap_match,
svr_region_distance_summary / _histogram / _quantile, svr_region_compare, svr_region_compare_measure; the contract is in
include/svr_abi.h, the design in DESIGN.md 8t).  Literal and exact: the surface by erosion of the zero-padded mask, counts by
np.bincount, sums in Python integers, the quantile on the sorted values, the measurement as the float64 expressions of the header.
Masks are bool arrays [nz][ny][nx]; maps and labels uint32 arrays of that shape."""
import math
from fractions import Fraction

import numpy as np

from tests import distance_ref as dr
from tests import histogram_ref as hr
from tests import region_ref as rr

NONE = 0xFFFFFFFF
MAX_TOL = 8
A_EMPTY, B_EMPTY = 1, 2
SUMMARY_FIELDS = ("voxels", "none", "sum", "sum_root_q8", "max", "first_max", "within")


def surface(mask, element=6):
    """mask & ~erode(pad(mask, 1, False)): the voxels with a neighbour under the element that is unset or outside the volume"""
    mask = mask.astype(bool)
    p = np.pad(mask, 1, constant_values=False)
    e = p.copy()
    for off in rr.offsets(element):
        e &= rr.shifted(p, off)
    return mask & ~e[1:-1, 1:-1, 1:-1]


def overlap(a, b, domain=None):
    """(both, a_only, b_only, neither) among the voxels of the domain"""
    a, b = a.astype(bool), b.astype(bool)
    d = np.ones(a.shape, bool) if domain is None else domain.astype(bool)
    code = (2 * (~a).astype(np.int64) + (~b).astype(np.int64))[d]           # 0 both, 1 a only, 2 b only, 3 neither
    return tuple(int(t) for t in np.bincount(code, minlength=4))


def label_overlap(a, count_a, b, count_b):
    """np.uint32[count_a + 1][count_b + 1]; voxels with a label above its count are not counted"""
    sel = (a <= count_a) & (b <= count_b)
    cell = a[sel].astype(np.int64) * (count_b + 1) + b[sel].astype(np.int64)
    return np.bincount(cell, minlength=(count_a + 1) * (count_b + 1)).astype(np.uint32).reshape(count_a + 1, count_b + 1)


def overlap_match(table):
    """(best_b_for_a, best_a_for_b) as lists of Python ints: the largest Jaccard index by Fractions, ties to the lower label, 0 for none"""
    t = [[int(c) for c in row] for row in np.asarray(table)]
    size_a = [sum(row) for row in t]
    size_b = [sum(row[lb] for row in t) for lb in range(len(t[0]))]

    def best(own, others, cell, size_own, size_other):
        out = []
        for i in own:
            top, arg = Fraction(0), 0
            for k in others:
                inter = cell(i, k)
                if inter and Fraction(inter, size_own[i] + size_other[k] - inter) > top:
                    top, arg = Fraction(inter, size_own[i] + size_other[k] - inter), k
            out.append(arg)
        return out
    ra, rb = range(1, len(t)), range(1, len(t[0]))
    return best(ra, rb, lambda la, lb: t[la][lb], size_a, size_b), best(rb, ra, lambda lb, la: t[la][lb], size_b, size_a)


def isqrt_float(p):
    """floor(sqrt(p)) of a uint64 array, 0 <= p < 2^53, by np.sqrt on float64 (exact conversions) with a +-1 integer fix-up"""
    p = np.asarray(p, dtype=np.uint64)
    s = np.sqrt(p.astype(np.float64)).astype(np.uint64)
    s = np.where(s * s > p, s - np.uint64(1), s)
    s = np.where((s + np.uint64(1)) * (s + np.uint64(1)) <= p, s + np.uint64(1), s)
    assert np.all(s * s <= p) and np.all(p < (s + np.uint64(1)) * (s + np.uint64(1)))
    return s


def values_of(d2, mask=None):
    """(the values of the map over the mask, their linear indices), in index order"""
    flat = np.asarray(d2, dtype=np.uint32).reshape(-1)
    idx = np.arange(flat.size) if mask is None else np.flatnonzero(mask.astype(bool).reshape(-1))
    return flat[idx], idx


def summary(d2, mask=None, tolerances2=()):
    """svr_distance_summary as a dict of Python ints (within: a list of 8)"""
    v, idx = values_of(d2, mask)
    real = v != NONE
    vals = v[real].astype(np.uint64)
    s = {"voxels": len(vals), "none": int((~real).sum()), "sum": sum(int(t) for t in vals), "sum_root_q8": sum(int(t) for t in isqrt_float(vals << np.uint64(16))),
         "max": 0, "first_max": 0}
    if len(vals):
        s["max"] = int(vals.max())
        s["first_max"] = int(idx[real][int(np.argmax(vals))])            # argmax: the first index of the maximum
    s["within"] = [int((vals <= np.uint64(tol)).sum()) for tol in tolerances2] + [0] * (MAX_TOL - len(tolerances2))
    return s


def histogram(d2, mask=None, lo=0, hi=65535, shift=0):
    """np.uint32[((hi - lo) >> shift) + 1]: values outside lo .. hi are not counted"""
    v, _ = values_of(d2, mask)
    v = v.astype(np.int64)
    v = v[(v >= lo) & (v <= hi)]
    return np.bincount((v - lo) >> shift, minlength=((hi - lo) >> shift) + 1).astype(np.uint32)


def quantile(d2, num, den, mask=None):
    """the inverted_cdf quantile of the values other than NONE, by histogram_ref.quantile on the sorted values; None when there is none"""
    v, _ = values_of(d2, mask)
    v = np.sort(v[v != NONE])
    if len(v) == 0:
        return None
    uniq, counts = np.unique(v, return_counts=True)
    return int(uniq[hr.quantile(counts, num, den)])


def compare(a, b, element=6, weights=(1, 1, 1), quantile_q=(95, 100), tolerances2=()):
    """svr_region_comparison as a dict: overlap (4), surface (2), ab / ba (summary dicts), quantile_ab / _ba, ntol, status"""
    a, b = a.astype(bool), b.astype(bool)
    sa, sb = surface(a, element), surface(b, element)
    out = {"overlap": list(overlap(a, b)), "surface": [int(sa.sum()), int(sb.sum())], "ntol": len(tolerances2),
           "status": (0 if a.any() else A_EMPTY) | (0 if b.any() else B_EMPTY)}
    for name, src, dst in (("ab", sa, sb), ("ba", sb, sa)):
        d2 = dr.distance_map(dst, weights, dr.TO_SET)
        out[name] = summary(d2, src, tolerances2)
        out["quantile_" + name] = quantile(d2, quantile_q[0], quantile_q[1], src) or 0
    return out


def directed_brute(a_surface, b_surface, weights=(1, 1, 1)):
    """the squared distances of every voxel of a_surface to the nearest of b_surface, by all pairs, in index order; None if b is empty"""
    p, t = np.argwhere(a_surface).astype(np.int64), np.argwhere(b_surface).astype(np.int64)
    if len(t) == 0:
        return None
    w = np.array([weights[2], weights[1], weights[0]], dtype=np.int64)       # (z, y, x)
    return [int(((t - q) ** 2 * w).sum(axis=1).min()) for q in p]


def measure(c, unit=1.0):
    """svr_compare_measurement as a dict of floats from the dict of compare(): the expressions of include/svr_abi.h in float64"""
    f = float
    nan = math.nan
    both, a_only, b_only = (f(c["overlap"][k]) for k in range(3))
    va, vb, uni = both + a_only, both + b_only, both + a_only + b_only
    n_ab, n_ba = f(c["ab"]["voxels"]), f(c["ba"]["voxels"])
    n = n_ab + n_ba
    m = {"dice": 2.0 * both / (2.0 * both + a_only + b_only) if uni > 0 else nan,
         "jaccard": both / uni if uni > 0 else nan,
         "volume_difference": 2.0 * (va - vb) / (va + vb) if va + vb > 0 else nan,
         "hausdorff_ab": unit * math.sqrt(f(c["ab"]["max"])) if n_ab > 0 else nan,
         "hausdorff_ba": unit * math.sqrt(f(c["ba"]["max"])) if n_ba > 0 else nan,
         "hausdorff_q_ab": unit * math.sqrt(f(c["quantile_ab"])) if n_ab > 0 else nan,
         "hausdorff_q_ba": unit * math.sqrt(f(c["quantile_ba"])) if n_ba > 0 else nan,
         "assd": unit * (f(c["ab"]["sum_root_q8"]) + f(c["ba"]["sum_root_q8"])) / 256.0 / n if n > 0 else nan,
         "rms": unit * math.sqrt((f(c["ab"]["sum"]) + f(c["ba"]["sum"])) / n) if n > 0 else nan}
    two = n_ab > 0 and n_ba > 0
    m["hausdorff"] = max(m["hausdorff_ab"], m["hausdorff_ba"]) if two else nan
    m["hausdorff_q"] = max(m["hausdorff_q_ab"], m["hausdorff_q_ba"]) if two else nan
    surf = f(c["surface"][0]) + f(c["surface"][1])
    m["surface_dice"] = [(f(c["ab"]["within"][k]) + f(c["ba"]["within"][k])) / surf if surf > 0 else nan for k in range(c["ntol"])] + \
                        [0.0] * (MAX_TOL - c["ntol"])
    return m


def summary_of_struct(s):
    """an abi.DistanceSummary as the dict of summary()"""
    return {"voxels": int(s.voxels), "none": int(s.none), "sum": int(s.sum), "sum_root_q8": int(s.sum_root_q8), "max": int(s.max),
            "first_max": int(s.first_max), "within": [int(t) for t in s.within]}


def comparison_of_struct(c):
    """an abi.RegionComparison as the dict of compare()"""
    return {"overlap": [int(t) for t in c.overlap], "surface": [int(t) for t in c.surface], "ab": summary_of_struct(c.ab), "ba": summary_of_struct(c.ba),
            "quantile_ab": int(c.quantile_ab), "quantile_ba": int(c.quantile_ba), "ntol": int(c.ntol), "status": int(c.status)}


def struct_of_comparison(c):
    """the dict of compare() as an abi.RegionComparison"""
    from sunvolumerender_amd import abi
    out = abi.RegionComparison()
    for k in range(4):
        out.overlap[k] = c["overlap"][k]
    out.surface[0], out.surface[1] = c["surface"]
    for name in ("ab", "ba"):
        s = getattr(out, name)
        for field in SUMMARY_FIELDS[:-1]:
            setattr(s, field, c[name][field])
        for k in range(MAX_TOL):
            s.within[k] = c[name]["within"][k]
    out.quantile_ab, out.quantile_ba, out.ntol, out.status = c["quantile_ab"], c["quantile_ba"], c["ntol"], c["status"]
    return out
