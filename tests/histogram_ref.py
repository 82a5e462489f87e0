"""The numpy / Python-int reference of the histogram calls (svr_volume_histogram, svr_region_label_histogram, svr_histogram_*; the
contract is in include/svr_abi.h, the design in DESIGN.md 8r).  Exact throughout: counts by np.bincount on the selected voxels, the
quantile by integer comparisons on the cumulative sum, Otsu by brute force over every threshold tuple with fractions.Fraction."""
from fractions import Fraction
from itertools import combinations

import numpy as np


def bins(lo=0, hi=65535, shift=0):
    return ((hi - lo) >> shift) + 1


def bin_range(b, lo=0, hi=65535, shift=0):
    """the raw values (first, last) of bin b"""
    return lo + (b << shift), min(hi, lo + ((b + 1) << shift) - 1)


def selected(u16, mask=None, lo=0, hi=65535, box=None):
    """bool [nz][ny][nx]: the voxels that count -- inside the inclusive box ((x0, y0, z0), (x1, y1, z1)) cut to the volume, mask set, lo <= v <= hi"""
    nz, ny, nx = u16.shape
    sel = (u16 >= lo) & (u16 <= hi)
    if mask is not None:
        sel &= mask.astype(bool)
    if box is not None:
        (x0, y0, z0), (x1, y1, z1) = box
        inside = np.zeros(u16.shape, bool)
        inside[max(z0, 0):min(z1, nz - 1) + 1, max(y0, 0):min(y1, ny - 1) + 1, max(x0, 0):min(x1, nx - 1) + 1] = True
        sel &= inside
    return sel


def histogram(u16, mask=None, lo=0, hi=65535, shift=0, box=None):
    """np.uint32[bins]"""
    sel = selected(u16, mask, lo, hi, box)
    b = (u16[sel].astype(np.int64) - lo) >> shift
    return np.bincount(b, minlength=bins(lo, hi, shift)).astype(np.uint32)


def label_histogram(labels, u16, count, lo=0, hi=65535, shift=0, box=None):
    """np.uint32[count + 1][bins]; labels above count are ignored"""
    nb = bins(lo, hi, shift)
    sel = selected(u16, None, lo, hi, box) & (labels <= count)
    cell = labels[sel].astype(np.int64) * nb + ((u16[sel].astype(np.int64) - lo) >> shift)
    return np.bincount(cell, minlength=(count + 1) * nb).astype(np.uint32).reshape(count + 1, nb)


def moments(counts):
    """(n, sum, sum_sq) of the bin indices, Python integers"""
    c = [int(t) for t in counts]
    return sum(c), sum(b * t for b, t in enumerate(c)), sum(b * b * t for b, t in enumerate(c))


def quantile(counts, num, den):
    """the smallest bin b with C(b) > 0 and den * C(b) >= num * N; None for an empty histogram"""
    c = [int(t) for t in counts]
    total, run = sum(c), 0
    if total == 0:
        return None
    for b, t in enumerate(c):
        run += t
        if run > 0 and den * run >= num * total:
            return b
    raise AssertionError("unreachable")


def otsu_criterion(counts, thresholds):
    """sum_j S_j^2 / N_j over the classes that `thresholds` (the last bins of the lower classes) cut, as a Fraction; an empty class gives 0"""
    c = [int(t) for t in counts]
    edges = [-1] + list(thresholds) + [len(c) - 1]
    total = Fraction(0)
    for a, b in zip(edges[:-1], edges[1:]):
        n = sum(c[a + 1:b + 1])
        s = sum(i * c[i] for i in range(a + 1, b + 1))
        if n:
            total += Fraction(s * s, n)
    return total


def otsu(counts, classes=2):
    """(thresholds, eta): the lexicographically smallest tuple t_1 < ... < t_{classes - 1} in 0 .. bins - 2 that maximises the criterion,
    and between-class / total variance as a float; (None, 0.0) for an empty histogram.  Brute force on prefix sums, exact."""
    c = [int(t) for t in counts]
    nb = len(c)
    cn, cs = [0], [0]
    for i, t in enumerate(c):
        cn.append(cn[-1] + t)
        cs.append(cs[-1] + i * t)
    n_all, s_all = cn[-1], cs[-1]
    if n_all == 0:
        return None, 0.0
    best, best_t = None, None
    for t in combinations(range(nb - 1), classes - 1):                   # lexicographic order: the first maximum is the smallest tuple
        edges = (-1,) + t + (nb - 1,)
        value = Fraction(0)
        for a, b in zip(edges[:-1], edges[1:]):
            n, s = cn[b + 1] - cn[a + 1], cs[b + 1] - cs[a + 1]
            if n:
                value += Fraction(s * s, n)
        if best is None or value > best:
            best, best_t = value, t
    ss = sum(i * i * t for i, t in enumerate(c))
    total = Fraction(ss) - Fraction(s_all * s_all, n_all)
    eta = float((best - Fraction(s_all * s_all, n_all)) / total) if total > 0 else 0.0
    return best_t, eta


def otsu2_fast(counts):
    """Two-class Otsu of a long histogram, exact and in one pass (integers: compare D^2 / (N1 N2), D = N S1 - N1 S, by
    cross-multiplication); the same answer as otsu(counts, 2)[0][0], for the 65536-bin cases where Fractions are slow"""
    c = [int(t) for t in counts]
    n_all, s_all = sum(c), sum(i * t for i, t in enumerate(c))
    if n_all == 0:
        return None
    best_num, best_den, best_t = 0, 1, 0
    n1 = s1 = 0
    for t in range(len(c) - 1):
        n1 += c[t]
        s1 += t * c[t]
        n2 = n_all - n1
        if n1 == 0 or n2 == 0:
            continue
        d = n_all * s1 - n1 * s_all
        if d * d * best_den > best_num * n1 * n2:
            best_num, best_den, best_t = d * d, n1 * n2, t
    return best_t


def otsu2_float(counts):
    """The textbook float Otsu: w0 w1 (m0 - m1)^2 in float64, first maximum"""
    c = np.asarray(counts, np.float64)
    idx = np.arange(len(c), dtype=np.float64)
    w0 = np.cumsum(c)[:-1]
    w1 = c.sum() - w0
    s0 = np.cumsum(c * idx)[:-1]
    s1 = (c * idx).sum() - s0
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where((w0 > 0) & (w1 > 0), w0 * w1 * (s0 / w0 - s1 / w1) ** 2, 0.0)
    return int(np.argmax(var))
