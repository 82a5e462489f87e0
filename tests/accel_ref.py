"""The skipping tables of csrc/svr_accel.hip restated in numpy, from their DEFINITIONS (the comments of that file and of
include/svr_abi.h), not from the kernels: tests/test_accel_gpu.py compares every entry of every device-built table with these for
equality, tests/test_accel_cpu.py anchors them on the oracle's own sampler (no alpha the oracle can return at a point exceeds the
bound of the point's cell).  There is no tolerance anywhere: the tables are integers, and the few float32 operations that
enter them (two multiplies, one fma, one product with invSigmaMax, the conversion of a random word) are reproduced with their
rounding.

Arrays of cells are indexed [z][y][x] like the volume; flat cell indices are x + gx (y + gy z), the kernels' order."""
from __future__ import annotations

import dataclasses
from fractions import Fraction
from typing import Optional

import numpy as np

f32 = np.float32

# capacities and layout of the device buffer (csrc/svr_kernels.hpp)
MASK_WORDS_MAX = 8192                      # one bit per macro-cell: at most 64^3 cells
DIST_WORDS_MAX = 4096                      # one nibble per half-resolution cell: at most 32^3
DIST_CAP = 15
BOUND_CLASSES = 16
BOUND8_DIM = 34
BOUND8_BYTES = 40960
OFF_DIST, OFF_DEEP, OFF_EMPTY = 0, DIST_WORDS_MAX, DIST_WORDS_MAX + MASK_WORDS_MAX
OFF_CLASS = DIST_WORDS_MAX + 2 * MASK_WORDS_MAX
OFF_THR = OFF_CLASS + DIST_WORDS_MAX
OFF_CENSUS = OFF_THR + BOUND_CLASSES
ACCEL_WORDS = OFF_CENSUS + 4
INV_65535 = f32(1.5259021896696422e-05)    # the sampler's scale of a raw u16 value


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the grid rule
def macro_grid(nx, ny, nz, shift_min=0):
    """(shift, (gx, gy, gz), (hgx, hgy, hgz)): the smallest shift >= shift_min whose grid has at most MASK_WORDS_MAX * 32 cells and
    whose half-resolution grid has at most DIST_WORDS_MAX * 8."""
    sh = shift_min
    while True:
        g = tuple(((n - 1) >> sh) + 1 for n in (nx, ny, nz))
        hg = tuple((c + 1) // 2 for c in g)
        if g[0] * g[1] * g[2] <= MASK_WORDS_MAX * 32 and hg[0] * hg[1] * hg[2] <= DIST_WORDS_MAX * 8:
            return sh, g, hg
        sh += 1


# ------------------------------------------------------------------------------------------------ min / max tables
def _axis_minmax(lo, hi, axis, n, S, g, pad):
    """Reduce axis `axis` (n voxels) of the running (min, max) pair to g cells: cell m takes voxels [m S - 1 - pad, m S + S - 1 + pad],
    one more on the last cell; voxels outside the volume are border texels, 0."""
    lo, hi = np.moveaxis(lo, axis, 0), np.moveaxis(hi, axis, 0)
    out_lo = np.empty((g,) + lo.shape[1:], dtype=lo.dtype)
    out_hi = np.empty_like(out_lo)
    for m in range(g):
        a, b = m * S - 1 - pad, m * S + S - 1 + pad + (1 if m == g - 1 else 0)      # inclusive
        ia, ib = max(a, 0), min(b, n - 1)
        outside = a < 0 or b > n - 1
        if ia <= ib:
            l, h = lo[ia:ib + 1].min(axis=0), hi[ia:ib + 1].max(axis=0)
            if outside:
                l, h = np.minimum(l, 0), np.maximum(h, 0)
        else:
            l, h = np.zeros(lo.shape[1:], lo.dtype), np.zeros(lo.shape[1:], lo.dtype)
        out_lo[m], out_hi[m] = l, h
    return np.moveaxis(out_lo, 0, axis), np.moveaxis(out_hi, 0, axis)


def minmax_table(vox, S, grid, pad=0):
    """(gz, gy, gx, 2) uint16: min and max of the raw voxels over the footprint of every cell of S voxels per axis.  A box footprint:
    the min / max over it is the min / max per axis in turn."""
    nz, ny, nx = vox.shape
    lo = hi = np.ascontiguousarray(vox, dtype=np.uint16)
    for axis, n, g in ((2, nx, grid[0]), (1, ny, grid[1]), (0, nz, grid[2])):
        lo, hi = _axis_minmax(lo, hi, axis, n, S, g, pad)
    return np.stack([lo, hi], axis=-1)


# ------------------------------------------------------------------------------------------------ raw value -> LUT entries
_COORD_CACHE: dict = {}


def lut_floor_of_raw(density_scale, tf_n):
    """floor of the transfer-function look-up coordinate of every raw u16 value, int64[65536]: I = (float32(r) * 1/65535) * densityScale
    (two float32 multiplies), x = clamp(fma(I, n, -0.5), -1, n), floor(x).

    The fma is evaluated in float64 and rounded once to float32.  Why the floor cannot differ from an exactly rounded fma: I n is exact
    in float64 (24 x 11 significant bits).  Where |I n| >= 2^-18 its last bit is at least 2^-18-34 = 2^-52, so I n - 0.5 is exact in
    float64 too and the single rounding to float32 IS the fma.  Below that, I n - 0.5 lies within 2^-18 of -0.5, every rounding of it
    stays inside (-1, 0), and the floor is -1 either way.  (tests/test_accel_cpu.py checks the table against rational arithmetic.)"""
    key = (float(f32(density_scale)), int(tf_n))
    if key not in _COORD_CACHE:
        r = np.arange(65536, dtype=np.float32)
        I = ((r * INV_65535).astype(np.float32) * f32(density_scale)).astype(np.float32)
        x = (I.astype(np.float64) * float(tf_n) - 0.5).astype(np.float32)
        x = np.minimum(np.maximum(x, f32(-1.0)), f32(tf_n))
        _COORD_CACHE[key] = np.floor(x).astype(np.int64)
    return _COORD_CACHE[key]


def lut_floor_exact(r, density_scale, tf_n):
    """lut_floor_of_raw for one raw value in rational arithmetic: the exact fma result v, rounded to the nearest float32 (ties to
    even), clamped, floored."""
    I = f32(f32(f32(r) * INV_65535) * f32(density_scale))
    v = Fraction(float(I)) * tf_n - Fraction(1, 2)
    k = v.numerator // v.denominator                           # floor of the exact value
    up = f32(k + 1)                                            # the float32 above: does v round up to it?
    if float(up) == k + 1:                                     # (representable: |k| < 2^24 here)
        below = np.nextafter(up, f32(-np.inf))
        mid = (Fraction(float(below)) + Fraction(float(up))) / 2
        even_up = (int(np.array(up).view(np.uint32)) & 1) == 0
        if v > mid or (v == mid and even_up):
            k += 1
    return int(min(max(k, -1), tf_n))


def padded_alpha(tf_rgba):
    """The alpha table as a look-up sees it: entry e (0 .. n + 2) is the alpha of texel clamp(e - 1, 0, n - 1); a look-up whose
    coordinate has floor f interpolates entries f + 1 and f + 2."""
    a = np.asarray(tf_rgba, dtype=np.float32).reshape(-1, 4)[:, 3]
    n = a.shape[0]
    return a[np.clip(np.arange(n + 3) - 1, 0, n - 1)]


class _RangeMax:
    """max over index ranges [lo, hi] of a fixed array (sparse table)."""

    def __init__(self, a):
        self.levels = [np.asarray(a)]
        k = 1
        while 2 * k <= len(a):
            p = self.levels[-1]
            self.levels.append(np.maximum(p[:-k], p[k:]))
            k *= 2

    def query(self, lo, hi):
        length = hi - lo + 1
        j = np.floor(np.log2(length)).astype(np.int64)
        out = np.empty(lo.shape, dtype=self.levels[0].dtype)
        for lv in np.unique(j):
            sel = j == lv
            t = self.levels[lv]
            out[sel] = np.maximum(t[lo[sel]], t[hi[sel] - (1 << int(lv)) + 1])
        return out


def cell_alpha_bounds(mm, tf_rgba, density_scale):
    """For every cell of a min/max table: (empty, A, bad).  The look-ups a fetch inside the cell can make touch the padded entries
    e_lo .. e_hi = floor(x(lowest intensity)) + 1 .. floor(x(highest intensity)) + 2 (a negative densityScale reverses the raw
    values' order).  empty: every one of those alphas is exactly 0.  A: the largest of them (at least 0).  bad: one of them is not a
    number -- no bound exists."""
    pa = padded_alpha(tf_rgba)
    n = len(pa) - 3
    fl = lut_floor_of_raw(density_scale, n)
    fa, fb = fl[mm[..., 0].astype(np.int64)], fl[mm[..., 1].astype(np.int64)]
    e_lo, e_hi = np.minimum(fa, fb) + 1, np.maximum(fa, fb) + 2
    nan = np.isnan(pa)
    nonzero_prefix = np.concatenate([[0], np.cumsum(~(pa == 0))])          # (a NaN is not zero)
    nan_prefix = np.concatenate([[0], np.cumsum(nan)])
    empty = (nonzero_prefix[e_hi + 1] - nonzero_prefix[e_lo]) == 0
    bad = (nan_prefix[e_hi + 1] - nan_prefix[e_lo]) > 0
    A = _RangeMax(np.where(nan, f32(0), np.maximum(pa, f32(0)))).query(e_lo, e_hi).astype(np.float32)
    return empty, A, bad


# ------------------------------------------------------------------------------------------------ bound classes, bound bytes
def class_thresholds():
    """thr[0] = 0, thr[c] = 2^((c - 15) / 2) for c = 1 .. 14 in float32 (a power of two, times float32(sqrt 2) for odd exponents),
    thr[15] = +inf."""
    thr = np.zeros(BOUND_CLASSES, dtype=np.float32)
    for c in range(1, BOUND_CLASSES - 1):
        k = 15 - c
        p = f32(2.0) ** f32(-((k + 1) // 2))
        thr[c] = f32(p * f32(1.41421356237)) if k & 1 else p
    thr[BOUND_CLASSES - 1] = np.inf
    return thr


def inv_sigma_max(max_opacity):
    return f32(1.0) / f32(max_opacity)


def accept_bound(A, bad, max_opacity):
    """b = float32(A) * float32(1 / maxOpacity), the product of the accept test; bad where it is not a number."""
    with np.errstate(invalid="ignore", over="ignore"):
        b = (A.astype(np.float32) * inv_sigma_max(max_opacity)).astype(np.float32)
    return b, bad | np.isnan(b)


def bound_class(b, bad):
    """the smallest class c with b <= thr[c]; 15 where there is no bound"""
    c = np.searchsorted(class_thresholds(), np.where(bad, f32(0), b), side="left").astype(np.uint32)
    return np.where(bad, np.uint32(BOUND_CLASSES - 1), c)


def word_to_uniform(x):
    """The accept draw of a random word: float32(x) (round to nearest even), then ONE exactly rounded fma(., 2^-32, 2^-33).  In float64
    the product and the sum are exact (a 24-bit integer times 2^-32, plus 2^-33: a multiple of 2^-33 below 2^34 of them), so the
    single rounding to float32 is the fma's."""
    fx = np.asarray(x, dtype=np.uint64).astype(np.float32)
    return (fx.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)


def bound_byte(b, bad):
    """B = min(255, X(b) >> 24), X(b) = the smallest word whose draw is >= b (2^32 if none), by bisection on the monotone conversion;
    255 where there is no bound."""
    b = np.asarray(b, dtype=np.float32)
    lo = np.zeros(b.shape, dtype=np.int64)
    hi = np.full(b.shape, 1 << 32, dtype=np.int64)
    for _ in range(33):
        active = lo < hi
        mid = (lo + hi) >> 1
        ge = word_to_uniform(np.minimum(mid, (1 << 32) - 1)) >= b
        hi = np.where(active & ge, mid, hi)
        lo = np.where(active & ~ge, mid + 1, lo)
    assert np.all(lo == hi)
    return np.where(bad, 255, np.minimum(255, lo >> 24)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ distances
def chebyshev_distance(nonempty):
    """D(c) = Chebyshev distance, in cells, from c to the nearest True cell of the grid, capped at DIST_CAP (cells outside the grid
    hold nothing).  The definition evaluated radius by radius: D(c) = the smallest r whose cube [c - r, c + r]^3, clipped to the grid,
    holds a True cell -- counted with a summed-volume table; no separable min-of-max construction."""
    ne = np.asarray(nonempty, dtype=bool)
    gz, gy, gx = ne.shape
    sat = np.zeros((gz + 1, gy + 1, gx + 1), dtype=np.int64)
    sat[1:, 1:, 1:] = ne.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    z, y, x = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    D = np.full(ne.shape, DIST_CAP, dtype=np.uint8)
    found = np.zeros(ne.shape, dtype=bool)
    for r in range(DIST_CAP):
        z0, z1 = np.maximum(z - r, 0), np.minimum(z + r, gz - 1) + 1
        y0, y1 = np.maximum(y - r, 0), np.minimum(y + r, gy - 1) + 1
        x0, x1 = np.maximum(x - r, 0), np.minimum(x + r, gx - 1) + 1
        cnt = (sat[z1, y1, x1] - sat[z0, y1, x1] - sat[z1, y0, x1] - sat[z1, y1, x0]
               + sat[z0, y0, x1] + sat[z0, y1, x0] + sat[z1, y0, x0] - sat[z0, y0, x0])
        hit = (cnt > 0) & ~found
        D[hit] = r
        found |= hit
    return D


def chebyshev_distance_brute(nonempty):
    """The same by the plainest means (every cell against every True cell): for small grids, to check the one above."""
    ne = np.asarray(nonempty, dtype=bool)
    pts = np.argwhere(ne)
    cells = np.argwhere(np.ones_like(ne))
    if len(pts) == 0:
        return np.full(ne.shape, DIST_CAP, dtype=np.uint8)
    d = np.abs(cells[:, None, :] - pts[None, :, :]).max(axis=2).min(axis=1)
    return np.minimum(d, DIST_CAP).astype(np.uint8).reshape(ne.shape)


def chebyshev_distance_separable(nonempty):
    """The construction the device uses (x, then y, then z: min over the offset o, |o| <= 14, of max(|o|, previous)), restated here
    only so that a CPU test can show it equals the definition."""
    ne = np.asarray(nonempty, dtype=bool)
    d = np.where(ne, 0, DIST_CAP).astype(np.int64)
    for axis in (2, 1, 0):
        n = d.shape[axis]
        best = np.full(d.shape, DIST_CAP, dtype=np.int64)
        for o in range(-(DIST_CAP - 1), DIST_CAP):
            src = np.full(d.shape, DIST_CAP, dtype=np.int64)       # outside the grid: infinitely far
            sl_dst, sl_src = [slice(None)] * 3, [slice(None)] * 3
            if o >= 0:
                sl_dst[axis], sl_src[axis] = slice(0, max(n - o, 0)), slice(o, n)
            else:
                sl_dst[axis], sl_src[axis] = slice(-o, n), slice(0, max(n + o, 0))
            src[tuple(sl_dst)] = d[tuple(sl_src)]
            best = np.minimum(best, np.maximum(src, abs(o)))
        d = best
    return d.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ half resolution, packing
def half_reduce(a, hg, op, fill):
    """op (np.minimum / np.maximum) over the in-grid 2 x 2 x 2 children of every half-resolution cell; `fill` is neutral for op."""
    gz, gy, gx = a.shape
    p = np.full((2 * hg[2], 2 * hg[1], 2 * hg[0]), fill, dtype=a.dtype)
    p[:gz, :gy, :gx] = a
    out = None
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                c = p[dz::2, dy::2, dx::2]
                out = c if out is None else op(out, c)
    return out


def pack_bits(flags, words=None):
    """bit (m & 31) of word m >> 5"""
    f = np.asarray(flags, dtype=bool).ravel()
    n = ceil_div(len(f), 32)
    padded = np.zeros(n * 32, dtype=np.uint64)
    padded[:len(f)] = f
    w = (padded.reshape(n, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    if words is not None:
        w = np.concatenate([w, np.zeros(words - n, dtype=np.uint32)])
    return w


def pack_nibbles(vals, words=None):
    """nibble (q & 7) of word q >> 3"""
    v = np.asarray(vals).ravel().astype(np.uint64)
    n = ceil_div(len(v), 8)
    padded = np.zeros(n * 8, dtype=np.uint64)
    padded[:len(v)] = v
    w = (padded.reshape(n, 8) << (4 * np.arange(8, dtype=np.uint64))).sum(axis=1).astype(np.uint32)
    if words is not None:
        w = np.concatenate([w, np.zeros(words - n, dtype=np.uint32)])
    return w


# ------------------------------------------------------------------------------------------------ everything together
@dataclasses.dataclass
class VolumeTables:
    """What depends on the voxels and the grid alone."""
    dim: tuple                  # (nx, ny, nz)
    shift: int
    grid: tuple                 # (gx, gy, gz)
    hgrid: tuple
    fgrid: Optional[tuple]      # the fine level (cells of half the edge) exists for shift >= 1
    mm: np.ndarray
    mm_fine: Optional[np.ndarray]
    mm_wide: np.ndarray         # half-resolution cells, footprints one voxel wider per side


def volume_tables(vox, shift_min=0) -> VolumeTables:
    nz, ny, nx = vox.shape
    shift, g, hg = macro_grid(nx, ny, nz, shift_min)
    fg = tuple(((n - 1) >> (shift - 1)) + 1 for n in (nx, ny, nz)) if shift >= 1 else None
    return VolumeTables((nx, ny, nz), shift, g, hg, fg, minmax_table(vox, 1 << shift, g),
                        minmax_table(vox, 1 << (shift - 1), fg) if fg else None, minmax_table(vox, 2 << shift, hg, pad=1))


@dataclasses.dataclass
class AccelTables:
    vt: VolumeTables
    empty: np.ndarray           # bool per macro-cell
    A: np.ndarray               # float32 per macro-cell: the largest alpha a fetch inside can return (+inf: no bound, a NaN entry)
    cls: np.ndarray             # bound class per macro-cell
    hcls: np.ndarray            # ... per half-resolution cell (largest child)
    dist: np.ndarray            # uint8 per macro-cell
    deep: np.ndarray            # bool
    hdist: np.ndarray           # per half-resolution cell (smallest child)
    fine_empty: Optional[np.ndarray]
    sub8: Optional[np.ndarray]
    bnd8: Optional[np.ndarray]  # BOUND8_BYTES, or None where the half-resolution grid has more than 32 cells on an axis
    A_wide: np.ndarray
    census: tuple               # (half-resolution cells of class 1..14, of class 15, empty macro-cells)

    @property
    def mask_words(self):
        return ceil_div(self.empty.size, 32)

    @property
    def dist_words(self):
        return ceil_div(self.hdist.size, 8)

    def accel_regions(self):
        """The device buffer region by region, each as far as it is DEFINED: the distance words and the `empty` words a kernel reads
        (dist_words, mask_words); the deep-empty and class regions whole (cleared beyond their data)."""
        return {
            "dist": (OFF_DIST, pack_nibbles(self.hdist)),
            "deep": (OFF_DEEP, pack_bits(self.deep, MASK_WORDS_MAX)),
            "empty": (OFF_EMPTY, pack_bits(self.empty)),
            "class": (OFF_CLASS, pack_nibbles(self.hcls, DIST_WORDS_MAX)),
            "thr": (OFF_THR, class_thresholds().view(np.uint32)),
            "census": (OFF_CENSUS, np.array(self.census, dtype=np.uint32)),
        }


def accel_tables(vt: VolumeTables, tf_rgba, density_scale, max_opacity) -> AccelTables:
    g, hg = vt.grid, vt.hgrid
    empty, A, bad = cell_alpha_bounds(vt.mm, tf_rgba, density_scale)
    cls = bound_class(*accept_bound(A, bad, max_opacity))
    hcls = half_reduce(cls, hg, np.maximum, np.uint32(0))
    dist = chebyshev_distance(~empty)
    hdist = half_reduce(dist, hg, np.minimum, np.uint8(DIST_CAP))
    fine_empty = sub8 = None
    if vt.fgrid is not None:
        fine_empty = cell_alpha_bounds(vt.mm_fine, tf_rgba, density_scale)[0]
        fz, fy, fx = fine_empty.shape
        sub8 = np.zeros(empty.shape, dtype=np.uint8)
        mz, my, mx = np.meshgrid(np.arange(g[2]), np.arange(g[1]), np.arange(g[0]), indexing="ij")
        for d in range(8):              # bit dx + 2 dy + 4 dz: that eighth is NOT empty; a child beyond the fine grid repeats its last cell
            child = fine_empty[np.minimum(2 * mz + (d >> 2), fz - 1), np.minimum(2 * my + ((d >> 1) & 1), fy - 1), np.minimum(2 * mx + (d & 1), fx - 1)]
            sub8 |= (~child).astype(np.uint8) << d
    _, A_wide, bad_wide = cell_alpha_bounds(vt.mm_wide, tf_rgba, density_scale)
    bnd8 = None
    if max(hg) + 2 <= BOUND8_DIM:
        byts = bound_byte(*accept_bound(A_wide, bad_wide, max_opacity))
        # entry (x + 1, y + 1, z + 1) = cell (x, y, z); every entry around the grid repeats the nearest edge cell
        cube = np.pad(byts, [(1, BOUND8_DIM - 1 - n) for n in (hg[2], hg[1], hg[0])], mode="edge")
        bnd8 = np.full(BOUND8_BYTES, 255, dtype=np.uint8)
        bnd8[:BOUND8_DIM ** 3] = cube.ravel()
    A, A_wide = np.where(bad, f32(np.inf), A), np.where(bad_wide, f32(np.inf), A_wide)      # (for the tests: no bound)
    census = (int(((hcls >= 1) & (hcls <= BOUND_CLASSES - 2)).sum()), int((hcls == BOUND_CLASSES - 1).sum()), int(empty.sum()))
    return AccelTables(vt, empty, A, cls, hcls, dist, dist >= 2, hdist, fine_empty, sub8, bnd8, A_wide, census)


# ------------------------------------------------------------------------------------------------ the test volumes and tables
def _hash01(shape, seed):
    """deterministic noise in [0, 1): an integer hash of the voxel index"""
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    h = (idx + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    return (h & np.uint64(0xFFFFFF)).astype(np.float64) / float(1 << 24)


def volume_37x21x10():
    """37 x 21 x 10 (no multiple of any cell size; odd grids at every shift).  Exact-zero air for x < 30: 30 empty macro-cells at shift 0 and
    15 at shift 1 (cells 0 .. 14 of 19; cell 15, voxels 29 .. 31, is the first that is not) -- the distance cap at both.  Then three voxels
    of low noise in two levels, raw 300 .. 900 for y < 16 and 3000 .. 4000 from y = 16 on (small alphas under the default table: two
    different middle classes, apart even in the 3 x 2 x 1 half-resolution grid of shift 3, whose cells (1, 0) and (1, 1) hold voxels
    15 .. 31 of x and -1 .. 15 / 15 .. 21 of y), then dense structure (x >= 33) that touches the faces x = 36, y = 0 / 20, z = 0 / 9
    with their edges and corners, with a planted air pocket inside it; the last voxel of every axis is non-zero."""
    nx, ny, nz = 37, 21, 10
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    noise = _hash01((nz, ny, nx), 3)
    v = np.where(x >= 30, np.where(y >= 16, 3000 + 1000 * noise, 300 + 600 * noise), 0.0)
    v = np.where(x >= 33, 20000 + 40000 * noise, v)
    v = np.where((x >= 33) & (x <= 35) & (y >= 6) & (y <= 14) & (z >= 2) & (z <= 7), 0.0, v)      # air pocket
    v[nz - 1, ny - 1, nx - 1] = 65535
    v[0, 0, nx - 1] = 50000
    return v.astype(np.uint16)


def volume_40x8x8():
    """40 x 8 x 8, one non-zero voxel at the far end of x: distances grow along x up to the cap and are limited by the grid's ends in y and z."""
    v = np.zeros((8, 8, 40), dtype=np.uint16)
    v[7, 7, 39] = 1500                    # (alpha 0.11 under the default table: a middle class)
    return v


def volume_64():
    """64^3 at shift 1: the 32^3 half-resolution grid, the largest with a byte table.  An exactly empty octant-and-more (x, y, z < 34), noise of
    every level elsewhere (a smooth ramp times a hash: many distinct bounds), dense blocks on faces, edges and corners."""
    n = 64
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    noise = _hash01((n, n, n), 7)
    ramp = (x + y + z) / (3.0 * (n - 1))
    v = 200 + 9000 * noise * ramp ** 2
    v = np.where((x < 34) & (y < 34) & (z < 34), 0.0, v)
    v = np.where((x >= 56) & (y >= 56), 30000 + 30000 * noise, v)
    v = np.where((z >= 60) & (x < 8), 45000.0, v)
    v[n - 1, n - 1, n - 1] = 65535
    v[0, n - 1, 0] = 12345
    return v.astype(np.uint16)


def default_tf():
    from sunvolumerender_amd import scenes
    return scenes.default_transfer_function()


def transfer_functions():
    """name -> (table, maxOpacity, densityScale): the tables of the GPU tests."""
    base, mo = default_tf()

    def with_alpha(a):
        t = base.copy()
        t[:, 3] = a
        return t

    hazy = np.maximum(base[:, 3] ** 3 / f32(0.25), f32(0.02)).astype(np.float32)      # alpha floor 0.02, a steep rise to 0.5
    nan = base[:, 3].copy()
    nan[40] = np.nan                                                                      # one entry that is not a number (raw ~ 2500)
    return {
        "default": (base, mo, 1.0),
        "transparent": (with_alpha(0.0), 0.5, 1.0),
        "opaque": (with_alpha(1.0), 1.0, 1.0),
        "hazy": (with_alpha(hazy), 0.5, 1.0),
        "dense_scale": (base, mo, 37.5),
        "nan_alpha": (with_alpha(nan), 0.5, 1.0),
        "negative_scale": (base, mo, -1.0),
    }


def volume_flat_512():
    """512 x 512 x 1, one slice: a disc of noisy tissue with a dense rim, exact-zero air around it, a dense bar along the edge x = 511."""
    y, x = np.meshgrid(np.arange(512), np.arange(512), indexing="ij")
    r = np.hypot(x - 250.0, y - 260.0)
    noise = _hash01((512, 512), 11)
    v = np.where(r < 180, 400 + 8000 * noise * (r / 180.0), 0.0)
    v = np.where((r >= 180) & (r < 190), 52000.0, v)
    v = np.where(x >= 504, 30000 + 20000 * noise, v)
    v[511, 511] = 65535
    return v.astype(np.uint16).reshape(1, 512, 512)


def volume_flat_1x400x330():
    """1 x 400 x 330 (nx = 1): the same kind of slice in the y-z plane."""
    z, y = np.meshgrid(np.arange(330), np.arange(400), indexing="ij")
    r = np.hypot(y - 190.0, z - 170.0)
    noise = _hash01((330, 400), 13)
    v = np.where(r < 120, 500 + 9000 * noise * (r / 120.0), 0.0)
    v = np.where((r >= 120) & (r < 128), 48000.0, v)
    v = np.where(z >= 324, 25000 + 20000 * noise, v)
    v[329, 399] = 65535
    return v.astype(np.uint16).reshape(330, 400, 1)


def volume_line_65538():
    """65538 x 1 x 1: air, a noisy ramp, a dense end."""
    x = np.arange(65538)
    noise = _hash01((65538,), 17)
    v = np.where(x >= 20000, 300 + 9000 * noise * (x - 20000) / 45538.0, 0.0)
    v = np.where((x >= 40000) & (x < 40400), 0.0, v)
    v = np.where(x >= 65000, 40000 + 20000 * noise, v)
    return v.astype(np.uint16).reshape(1, 1, 65538)


VOLUMES = {
    # name: (factory, SVR_OPT_MACRO_SHIFT_MIN)
    "37x21x10_s0": (volume_37x21x10, 0),
    "37x21x10_s1": (volume_37x21x10, 1),
    "37x21x10_s2": (volume_37x21x10, 2),
    "37x21x10_s3": (volume_37x21x10, 3),
    "40x8x8_s0": (volume_40x8x8, 0),
    "64_s1": (volume_64, 1),
    # flat and line-like volumes: their half-resolution grid, not the grid itself, decides the shift
    "flat_512x512x1": (volume_flat_512, 0),
    "flat_1x400x330": (volume_flat_1x400x330, 0),
    "line_65538x1x1": (volume_line_65538, 0),
}
SMALL_VOLUMES = [k for k in VOLUMES if k[0].isdigit()]
FLAT_VOLUMES = [k for k in VOLUMES if not k[0].isdigit()]

_VT_CACHE: dict = {}
_VOX_CACHE: dict = {}


def named_volume(name):
    """(voxels, VolumeTables) of a named test volume, computed once per session."""
    if name not in _VT_CACHE:
        factory, shift_min = VOLUMES[name]
        if factory not in _VOX_CACHE:
            _VOX_CACHE[factory] = factory()
        _VT_CACHE[name] = (_VOX_CACHE[factory], volume_tables(_VOX_CACHE[factory], shift_min))
    return _VT_CACHE[name]
