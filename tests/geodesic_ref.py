"""Test-side reference of the geodesic calls (include/svr_abi.h, "geodesic distances and influence zones"), numpy only and literal: every
voxel holds the packed key (dist << 32) | zone, and "take the minimum over yourself and key(u) + (w << 32) of your allowed neighbours u" is
iterated on all voxels at once (Jacobi) with the 26 shifted views and the weight of each move's class, to the fixpoint.  The split and the
zone cut are built from that, tests/distance_ref.py and tests/label_ref.py.  Nothing here knows about tiles, sweeps or dirty maps."""
import heapq
import itertools

import numpy as np

from tests import distance_ref as dr
from tests import label_ref as lr
from tests import region_ref as rr

NONE = 0xFFFFFFFF
LIMIT = 0xFFFFFFFE
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
CHAMFER = (3, 3, 3, 4, 4, 4, 5)
CLASSES = {6: 3, 18: 6, 26: 7}                           # the move classes a connectivity allows
_S32 = np.uint64(32)


def move_class(off):
    """The class (x, y, z, xy, xz, yz, xyz -> 0 .. 6) of a move (dz, dy, dx) from the coordinates it changes."""
    dz, dy, dx = off
    return {1: 0, 2: 1, 4: 2, 3: 3, 5: 4, 6: 5, 7: 6}[(dx != 0) | (dy != 0) << 1 | (dz != 0) << 2]


def moves(weights):
    """[((dz, dy, dx), w)] of the allowed moves."""
    out = []
    for off in itertools.product((-1, 0, 1), repeat=3):
        if any(off) and weights[move_class(off)]:
            out.append((off, int(weights[move_class(off)])))
    return out


def default_weights(connectivity):
    return tuple(w if c < CLASSES[connectivity] else 0 for c, w in enumerate(CHAMFER))


def fits(weights, shape):
    """The overflow bound of the contract: wmax (voxels - 1) <= 0xFFFFFFFE."""
    return max(int(w) for w in weights) * (int(np.prod([int(n) for n in shape], dtype=object)) - 1) <= LIMIT


def shifted_keys(key, off):
    """b[p] = key[p - off], KEY_NONE where p - off lies outside."""
    out = np.full_like(key, KEY_NONE)
    src, dst = [], []
    for o, n in zip(off, key.shape):
        if abs(o) >= n:
            return out
        src.append(slice(max(0, -o), n - max(0, o)))
        dst.append(slice(max(0, o), n - max(0, -o)))
    out[tuple(dst)] = key[tuple(src)]
    return out


def geodesic(labels, domain, weights=CHAMFER):
    """(dist, zones) as uint32 arrays [nz][ny][nx]."""
    labels = np.asarray(labels, dtype=np.uint32)
    domain = np.asarray(domain, dtype=bool)
    assert fits(weights, domain.shape) and any(weights)
    key = np.where(domain & (labels != 0), labels.astype(np.uint64), KEY_NONE)
    mv = moves(weights)
    while True:
        new = key.copy()
        for off, w in mv:
            s = shifted_keys(key, off)
            cand = np.where((s >> _S32) != np.uint64(NONE), s + (np.uint64(w) << _S32), KEY_NONE)
            np.minimum(new, cand, out=new)
        new[~domain] = KEY_NONE
        if np.array_equal(new, key):
            break
        key = new
    dist = (key >> _S32).astype(np.uint32)
    zones = np.where(dist != NONE, key & np.uint64(NONE), 0).astype(np.uint32)
    return dist, zones


def dijkstra(labels, domain, weights=CHAMFER):
    """The same pair by an independent method: a heap that pops (dist, label, voxel)."""
    nz, ny, nx = domain.shape
    dist = np.full(domain.shape, NONE, dtype=np.uint32)
    zones = np.zeros(domain.shape, dtype=np.uint32)
    done = np.zeros(domain.shape, dtype=bool)
    heap = [(0, int(labels[p]), p) for p in map(tuple, np.argwhere(domain & (labels != 0)).tolist())]
    heapq.heapify(heap)
    mv = moves(weights)
    while heap:
        d, lab, p = heapq.heappop(heap)
        if done[p]:
            continue
        done[p], dist[p], zones[p] = True, d, lab
        for (dz, dy, dx), w in mv:
            q = (p[0] + dz, p[1] + dy, p[2] + dx)
            if 0 <= q[0] < nz and 0 <= q[1] < ny and 0 <= q[2] < nx and domain[q] and not done[q]:
                heapq.heappush(heap, (d + w, lab, q))
    return dist, zones


def seed_labels(seeds, shape):
    """Label i + 1 on the voxel (x, y, z) of seed i; the lowest i of several on one voxel."""
    out = np.zeros(shape, dtype=np.uint32)
    for i, (x, y, z) in reversed(list(enumerate(seeds))):
        out[z, y, x] = i + 1
    return out


def split(mask, r2, connectivity=26, dist_weights=(1, 1, 1), step_weights=None):
    """(zones, K, unreached) of svr_region_split."""
    cores = dr.ball(mask, dr.ERODE, r2, dist_weights)
    labels, count = lr.label(cores, connectivity)
    _, zones = geodesic(labels, mask, default_weights(connectivity) if step_weights is None else step_weights)
    return zones, count, int((mask & (zones == 0)).sum())


def zone_cut(zones, connectivity=26):
    keep = zones != 0
    for off in rr.offsets(connectivity):
        n = rr.shifted(zones, off)                       # 0 outside the volume
        keep &= ~((n != 0) & (n < zones))
    return keep


def weights_at(spacing, connectivity, k):
    """The seven weights at unit = min(spacing) / 2^k: max(1, round half away from zero (len / unit)), 0 beyond the connectivity."""
    sx, sy, sz = (float(s) for s in spacing)
    lens = [sx, sy, sz, np.sqrt(sx * sx + sy * sy), np.sqrt(sx * sx + sz * sz), np.sqrt(sy * sy + sz * sz), np.sqrt(sx * sx + sy * sy + sz * sz)]
    unit = min(sx, sy, sz) / 2 ** k
    return tuple(max(1, int(np.floor(l / unit + 0.5))) if c < CLASSES[connectivity] else 0 for c, l in enumerate(lens)), unit


def weights_from_spacing(spacing, connectivity, shape):
    """((7 weights), unit, k) by the definition of svr_region_geodesic_weights; ValueError where it refuses."""
    if connectivity not in CLASSES or not all(np.isfinite(float(s)) and float(s) > 0 for s in spacing):
        raise ValueError("refused")
    for k in (3, 2, 1, 0):
        w, unit = weights_at(spacing, connectivity, k)
        if fits(w, shape):
            return w, unit, k
    raise ValueError("no k fits")


# ---------------------------------------------------------------------------------------------- fixtures shared by the CPU and GPU tests
TILE = (32, 8, 8)                                        # voxels of a relaxation tile (x, y, z): abi.GEO_TILE
GPU_SHAPE = (19, 21, 72)                                 # [nz][ny][nx]: three tiles on every axis, no dimension a multiple of the tile
DENSITIES = (0.7, 0.45)
WEIGHT_SETS = {"chamfer": CHAMFER, "6-only": (3, 3, 3, 0, 0, 0, 0), "18-only": (3, 3, 3, 4, 4, 4, 0), "distinct": (2, 3, 5, 4, 6, 7, 9)}
FLAT_SHAPES = [(1, 1, 33), (1, 1, 70), (1, 21, 1), (19, 1, 1), (1, 1, 1)]


def random_domain(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def random_markers(shape, n, seed):
    """n voxels anywhere in the volume with random labels from the whole non-zero 32-bit range."""
    rng = np.random.default_rng(seed)
    labels = np.zeros(shape, dtype=np.uint32)
    at = rng.choice(labels.size, min(n, labels.size), replace=False)
    labels.reshape(-1)[at] = rng.integers(1, 2 ** 32, len(at), dtype=np.uint64).astype(np.uint32)
    return labels


def random_case(density, seed=5):
    k = DENSITIES.index(density)
    return random_domain(GPU_SHAPE, density, seed + k), random_markers(GPU_SHAPE, 40, 100 + seed + k)


def tie_line(axis, middle, swapped, half=5):
    """A straight corridor of 2 * half + 1 voxels along `axis` (0 = x, 1 = y, 2 = z) of a GPU_SHAPE volume whose middle voxel has the
    coordinate `middle`, with label 7 at one end and 3 at the other (the other way round when swapped).  Returns (labels, domain, the
    (z, y, x) of the middle voxel)."""
    domain = np.zeros(GPU_SHAPE, dtype=bool)
    labels = np.zeros(GPU_SHAPE, dtype=np.uint32)
    p = [9, 10, 40]                                       # (z, y, x) of the line's fixed coordinates
    ax = 2 - axis
    lo, hi, mid = list(p), list(p), list(p)
    lo[ax], hi[ax], mid[ax] = middle - half, middle + half, middle
    sl = [slice(c, c + 1) for c in p]
    sl[ax] = slice(middle - half, middle + half + 1)
    domain[tuple(sl)] = True
    labels[tuple(lo)], labels[tuple(hi)] = (3, 7) if swapped else (7, 3)
    return labels, domain, tuple(mid)


TIE_CASES = [(axis, middle) for axis in (0, 1, 2) for middle in (TILE[axis] - 1, TILE[axis])]      # the tie voxel on each side of a tile face

SERPENTINE_SHAPE = (9, 40, 70)
SERPENTINE_SEED = (0, 0, 4)                              # (x, y, z)
SERPENTINE_MAX = 2863                                    # the largest chamfer distance in it


def serpentine():
    """A corridor two voxels high that winds through the volume: walls at y = 2, 5, 8, ... with gaps two voxels wide that alternate
    between the two x ends.  Returns (labels, domain) with one seed of label 9 at a corner."""
    nz, ny, nx = SERPENTINE_SHAPE
    domain = np.ones(SERPENTINE_SHAPE, dtype=bool)
    for i, y in enumerate(range(2, ny, 3)):
        domain[:, y, :] = False
        if i % 2 == 0:
            domain[:, y, nx - 2:] = True
        else:
            domain[:, y, :2] = True
    labels = np.zeros(SERPENTINE_SHAPE, dtype=np.uint32)
    x, y, z = SERPENTINE_SEED
    labels[z, y, x] = 9
    return labels, domain


PHANTOM_SHAPE = (24, 24, 40)
PHANTOM_R2 = 36                                          # d2_to_unset > 36 leaves two cores, > 25 one
PHANTOM_ZONES = {"chamfer": (3019, 2917), "6": (3024, 2912)}
PHANTOM_6_WEIGHTS = (1, 1, 1, 0, 0, 0, 0)
PHANTOM_R2_NONE = 100                                    # no voxel is farther than that from the outside: no core
THIN_R2, THIN_DIST_WEIGHTS = 4, (1, 1, 2)


def two_ball_phantom():
    """Two balls of squared radius 81 around (x, y, z) = (12, 12, 12) and (26, 11, 12) that overlap: one component with a neck."""
    zz, yy, xx = np.mgrid[:PHANTOM_SHAPE[0], :PHANTOM_SHAPE[1], :PHANTOM_SHAPE[2]]
    return ((xx - 12) ** 2 + (yy - 12) ** 2 + (zz - 12) ** 2 <= 81) | ((xx - 26) ** 2 + (yy - 11) ** 2 + (zz - 12) ** 2 <= 81)


def thin_pieces_mask():
    """Random points grown by the ball of r2 = 3 in a GPU_SHAPE volume: 25 components, of which the erosion by THIN_R2 under
    THIN_DIST_WEIGHTS leaves 12 cores; the pieces without a core stay unreached."""
    return dr.ball(dr.random_mask(GPU_SHAPE, 0.015, 9), dr.DILATE, 3)


def cached(key, make):
    return rr.cached(("geodesic",) + tuple(key), make)


def cached_geodesic(name, labels, domain, weights=CHAMFER):
    return cached((name, tuple(weights)), lambda: geodesic(labels, domain, weights))
