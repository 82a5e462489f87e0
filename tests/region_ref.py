"""Test-side reference of the region calls (include/svr_abi.h, "seeded region growing"), numpy only and literal: the region is grown by
iterating region |= dilate(region, structure) & candidates to the fixpoint, with the 6 / 18 / 26 structures as shifted-array ORs, and the
statistics -- the face counts included -- are computed from their definitions.  Nothing here knows about tiles, words or sweeps."""
import itertools

import numpy as np

OK, EMPTY = 0, 1
KEEP, REMOVE = 1, 2
STAT_INTS = ("voxels", "sum", "sum_sq", "sum_x", "sum_y", "sum_z", "faces_x", "faces_y", "faces_z", "vmin", "vmax", "bbox_min", "bbox_max",
             "status")


def offsets(connectivity):
    """(dz, dy, dx) of the neighbours: 1 non-zero component for 6, up to 2 for 18, up to 3 for 26."""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(c != 0 for c in o) <= most]


def shifted(a, off):
    """b[p] = a[p - off], False where p - off lies outside: the set `a` moved by `off`."""
    out = np.zeros_like(a)
    src, dst = [], []
    for o, n in zip(off, a.shape):
        if abs(o) >= n:
            return out
        src.append(slice(max(0, -o), n - max(0, o)))
        dst.append(slice(max(0, o), n - max(0, -o)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def candidates(vox, lo, hi, box=None):
    c = (vox >= lo) & (vox <= hi)
    if box is not None:
        (x0, y0, z0), (x1, y1, z1) = box
        inside = np.zeros_like(c)
        inside[max(z0, 0):z1 + 1, max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] = True
        c &= inside
    return c


def grow(vox, seeds, lo, hi, connectivity=6, box=None):
    """The region as a bool array [nz][ny][nx]; seeds are (x, y, z)."""
    cand = candidates(vox, lo, hi, box)
    region = np.zeros_like(cand)
    for x, y, z in seeds:
        if cand[z, y, x]:
            region[z, y, x] = True
    offs = offsets(connectivity)
    while True:
        d = region.copy()
        for o in offs:
            d |= shifted(region, o)
        d &= cand
        if np.array_equal(d, region):
            return region
        region = d


def stats(vox, region):
    """svr_region_stats as a dict of Python ints (bbox_min / bbox_max: lists in x, y, z order)."""
    nz, ny, nx = vox.shape
    n = int(region.sum())
    v = vox[region].astype(object)                       # Python integers: no overflow anywhere
    zz, yy, xx = np.nonzero(region)
    s = {"voxels": n, "sum": int(sum(v)), "sum_sq": int(sum(int(t) * int(t) for t in v)),
         "sum_x": int(xx.astype(np.int64).sum()), "sum_y": int(yy.astype(np.int64).sum()), "sum_z": int(zz.astype(np.int64).sum())}
    for name, off in (("faces_x", (0, 0, 1)), ("faces_y", (0, 1, 0)), ("faces_z", (1, 0, 0))):
        faces = 0
        for sgn in (1, -1):
            o = tuple(sgn * c for c in off)
            # the neighbour of p at p + o is in the region iff (region moved by -o)[p]; outside the volume counts as not
            faces += int((region & ~shifted(region, tuple(-c for c in o))).sum())
        s[name] = faces
    if n:
        s["vmin"], s["vmax"] = int(vox[region].min()), int(vox[region].max())
        s["bbox_min"] = [int(xx.min()), int(yy.min()), int(zz.min())]
        s["bbox_max"] = [int(xx.max()), int(yy.max()), int(zz.max())]
    else:
        s["vmin"], s["vmax"] = 65535, 0
        s["bbox_min"], s["bbox_max"] = [nx, ny, nz], [-1, -1, -1]
    s["status"] = OK if n else EMPTY
    return s


def pack(region):
    """The bit mask of the contract: uint32 words, voxel (x, y, z) = bit x & 31 of word (z * ny + y) * wx + (x >> 5), padding 0."""
    nz, ny, nx = region.shape
    wx = (nx + 31) // 32
    padded = np.zeros((nz, ny, wx * 32), dtype=np.uint8)
    padded[:, :, :nx] = region
    return np.packbits(padded, axis=-1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def unpack(words, shape):
    nz, ny, nx = shape
    wx = (nx + 31) // 32
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8).reshape(nz, ny, wx * 4), axis=-1, bitorder="little")
    return bits[:, :, :nx].astype(bool)


def apply(vox, region, mode, fill):
    keep = region if mode == KEEP else ~region
    return np.where(keep, vox, np.uint16(fill)).astype(np.uint16)


def measure(vox, region, spacing):
    """svr_region_measure from the voxels themselves, float64."""
    sx, sy, sz = (float(t) for t in spacing)
    st = stats(vox, region)
    n = st["voxels"]
    out = {"surface_area": st["faces_x"] * sy * sz + st["faces_y"] * sx * sz + st["faces_z"] * sx * sy}
    if n == 0:
        out.update(volume=0.0, mean=0.0, stddev=0.0, centroid=[0.0, 0.0, 0.0])
        return out
    v = vox[region].astype(np.float64)
    zz, yy, xx = np.nonzero(region)
    out.update(volume=n * sx * sy * sz, mean=float(v.mean()), stddev=float(v.std()),
               centroid=[float(xx.mean()), float(yy.mean()), float(zz.mean())])
    return out


# ---------------------------------------------------------------------------------------------- fixtures shared by the CPU and GPU tests
TILE = (128, 8, 8)                                       # voxels of a grow tile (x, y, z): 4 mask words x 8 rows x 8 slices
WORD = 32


def serpentine(shape=(17, 24, 40)):
    """A one-voxel corridor through a [nz][ny][nx] volume: rows along x on every second y, joined at alternating ends, on every second
    slice, the slices joined at alternating ends too.  Returns (vox, seed): corridor voxels are 1000, the rest 0."""
    nz, ny, nx = shape
    vox = np.zeros(shape, dtype=np.uint16)
    x_at = 0                                             # where the corridor stands
    for zi, z in enumerate(range(0, nz, 2)):
        ys = list(range(0, ny, 2))
        if zi % 2:
            ys.reverse()
        for yi, y in enumerate(ys):
            vox[z, y, :] = 1000
            x_at = (nx - 1) if x_at == 0 else 0          # the row is walked to its other end
            if yi + 1 < len(ys):
                vox[z, (y + ys[yi + 1]) // 2, x_at] = 1000
        if z + 2 < nz:
            vox[z + 1, ys[-1], x_at] = 1000
    return vox, (0, 0, 0)


_CACHE = {}


def cached(key, make):
    """One reference per key for the whole session; the arrays are read-only."""
    if key not in _CACHE:
        val = make()
        for a in (val if isinstance(val, tuple) else (val,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = val
    return _CACHE[key]


def reference(name, vox, seeds, lo, hi, connectivity=6, box=None):
    """(region, stats) of a named case, computed once."""
    def make():
        r = grow(vox, seeds, lo, hi, connectivity, box)
        return r, stats(vox, r)
    return cached((name, vox.shape, lo, hi, connectivity, tuple(map(tuple, seeds)), None if box is None else tuple(map(tuple, box))), make)


# the kernel's edge cases.  Shapes are (nz, ny, nx); one voxel less / exactly / one more than a mask word (32) and a tile (128 x 8 x 8)
EDGE_SHAPES = [(5, 7, 33), (3, 9, 65), (1, 1, 1), (1, 1, 64), (1, 40, 1), (1, 24, 40), (300, 8, 8),
               (7, 7, 31), (8, 8, 32), (9, 9, 33), (9, 7, 127), (8, 8, 128), (7, 9, 129), (17, 16, 256)]
NOISE_LO, NOISE_HI = 0, 649                              # the window of the noise volumes: 65 % of the voxels, above the percolation threshold


def noise_volume(shape, seed=7):
    """Uniform values 0 .. 999: the window 0 .. 649 gives one large cluster, many small ones and many non-candidates."""
    return np.random.default_rng(seed).integers(0, 1000, size=shape, dtype=np.uint16)


def spread_seeds(vox, lo=NOISE_LO, hi=NOISE_HI, n=3):
    """n candidate voxels (x, y, z) spread over the volume in scan order (fewer if there are fewer candidates)."""
    c = np.argwhere((vox >= lo) & (vox <= hi))
    if len(c) == 0:
        return [(0, 0, 0)]
    pick = sorted(set(int(round(t)) for t in np.linspace(0, len(c) - 1, n)))
    return [tuple(int(t) for t in c[i][::-1]) for i in pick]


PAIR_SHAPE = (20, 20, 160)
# (name, voxel A, voxel B) in (x, y, z): joined across an edge or across a corner only, on either side of the named boundary
PAIRS = [
    ("word-edge", (31, 3, 3), (32, 4, 3)), ("word-corner", (31, 3, 3), (32, 4, 4)),
    ("tiley-edge", (40, 7, 3), (41, 8, 3)), ("tiley-edge-yz", (40, 7, 3), (40, 8, 4)), ("tiley-corner", (40, 7, 3), (41, 8, 4)),
    ("tilez-edge", (40, 3, 7), (40, 4, 8)), ("tilez-edge-xz", (40, 3, 7), (41, 3, 8)), ("tilez-corner", (40, 3, 7), (41, 4, 8)),
    ("tilex-edge", (127, 3, 3), (128, 4, 3)), ("tilex-corner", (127, 3, 3), (128, 4, 4)),
    ("tilecorner-edge-xy", (127, 7, 7), (128, 8, 7)), ("tilecorner-edge-yz", (127, 7, 7), (127, 8, 8)),
    ("tilecorner-edge-xz", (127, 7, 7), (128, 7, 8)), ("tilecorner-corner", (127, 7, 7), (128, 8, 8)),
    ("tilecorner-corner-down", (128, 8, 8), (127, 9, 7)),
]


def pair_volume(a, b):
    vox = np.zeros(PAIR_SHAPE, dtype=np.uint16)
    vox[a[2], a[1], a[0]] = 1000
    vox[b[2], b[1], b[0]] = 1000
    return vox


def pair_expected(a, b, connectivity):
    """How many voxels the region from A holds: 2 iff the move A -> B is admitted."""
    k = sum(1 for p, q in zip(a, b) if p != q)
    return 2 if k <= {6: 1, 18: 2, 26: 3}[connectivity] else 1


def bridge_volume():
    """Two bars along y joined by a bridge at y = 17: the box y <= 15 cuts the region in two.  Returns (vox, seed, box)."""
    vox = np.zeros((10, 20, 40), dtype=np.uint16)
    vox[2:8, 1:19, 4:8] = 500
    vox[2:8, 1:19, 30:36] = 500
    vox[2:8, 17, 4:36] = 500
    return vox, (5, 3, 4), ((0, 0, 0), (39, 15, 9))
