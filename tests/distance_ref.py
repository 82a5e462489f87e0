"""Test-side reference of the distance calls (include/svr_abi.h, "exact Euclidean distance maps"), numpy only and literal: per axis
out[u] = min over i of g[i] + w (u - i)^2 by broadcasting in int64, with "no target" carried as a separate boolean and never as a big
number; ball, select, dmax, to_volume and weights follow their definitions.  Nothing here knows about words, envelopes or stacks.  Masks
are bool arrays [nz][ny][nx]; weights are (wx, wy, wz)."""
import math

import numpy as np

from tests import region_ref as rr

NONE = 0xFFFFFFFF
LIMIT = 0xFFFFFFFE
TO_SET, TO_UNSET = 1, 2
DILATE, ERODE, OPEN, CLOSE = 1, 2, 3, 4
OPS = (DILATE, ERODE, OPEN, CLOSE)
TARGETS = (TO_SET, TO_UNSET)


def fits(weights, shape):
    """The overflow bound of the contract, in Python integers."""
    nz, ny, nx = (int(n) for n in shape)
    wx, wy, wz = (int(w) for w in weights)
    return wx * (nx - 1) ** 2 + wy * (ny - 1) ** 2 + wz * (nz - 1) ** 2 <= LIMIT


def targets(mask, target):
    return mask if target == TO_SET else ~mask


def axis_pass(g, fin, w, axis):
    """(out, fin_out): out[u] = min over the i with fin[i] of g[i] + w (u - i)^2 along `axis`; fin_out says whether there was such an i."""
    g = np.moveaxis(g, axis, -1)
    fin = np.moveaxis(fin, axis, -1)
    n = g.shape[-1]
    idx = np.arange(n, dtype=np.int64)
    cost = int(w) * (idx[:, None] - idx[None, :]) ** 2                      # [u][i]
    # the minimum over the sites that exist; where there is none the entry is cleared and fin_out says so.  (In slabs of columns, so that
    # the [u][i] tables stay small.)
    lead = g.shape[:-1]
    g2, f2 = g.reshape(-1, n), fin.reshape(-1, n)
    out = np.empty_like(g2)
    slab = max(1, (1 << 19) // (n * n))
    for a in range(0, len(g2), slab):
        gs, fs = g2[a:a + slab], f2[a:a + slab]
        out[a:a + slab] = np.min(gs[:, None, :] + cost, axis=-1, where=fs[:, None, :], initial=np.iinfo(np.int64).max)
    out = np.where(f2.any(axis=-1, keepdims=True), out, 0).reshape(lead + (n,))
    fin_out = np.broadcast_to(fin.any(axis=-1, keepdims=True), g.shape)
    return np.moveaxis(out, -1, axis).astype(np.int64), np.moveaxis(fin_out, -1, axis).copy()


def distance(mask, weights=(1, 1, 1), target=TO_SET):
    """(d2, finite): int64 squared distances [nz][ny][nx] and where they exist (everywhere, or nowhere when there is no target)."""
    t = targets(mask, target)
    g, fin = np.zeros(mask.shape, dtype=np.int64), t.copy()
    for axis, w in ((2, weights[0]), (1, weights[1]), (0, weights[2])):
        g, fin = axis_pass(g, fin, w, axis)
    return np.where(fin, g, 0), fin


def as_map(d2, fin):
    """The map of the contract: uint32, SVR_DIST_NONE where there is no distance."""
    assert int(d2.max(initial=0)) <= LIMIT
    out = d2.astype(np.uint32)
    out[~fin] = NONE
    return out


def distance_map(mask, weights=(1, 1, 1), target=TO_SET):
    return as_map(*distance(mask, weights, target))


def brute(mask, weights=(1, 1, 1), target=TO_SET):
    """The same by all pairs: for small shapes only."""
    t = np.argwhere(targets(mask, target)).astype(np.int64)                # (z, y, x)
    fin = np.full(mask.shape, len(t) > 0)
    if len(t) == 0:
        return np.zeros(mask.shape, dtype=np.int64), fin
    p = np.argwhere(np.ones(mask.shape, dtype=bool)).astype(np.int64)
    wz, wy, wx = int(weights[2]), int(weights[1]), int(weights[0])
    d = p[:, None, :] - t[None, :, :]
    d2 = wz * d[..., 0] ** 2 + wy * d[..., 1] ** 2 + wx * d[..., 2] ** 2
    return d2.min(axis=1).reshape(mask.shape), fin


def dilate_of(to_set_map, r2):
    """The dilation from the TO_SET map: the voxels within r2 of a set voxel (none when there is no set voxel)."""
    return (to_set_map != NONE) & (to_set_map.astype(np.int64) <= r2)


def erode_of(to_unset_map, r2):
    """The erosion from the TO_UNSET map: the voxels further than r2 from every unset voxel of the volume (all when there is none)."""
    return (to_unset_map == NONE) | (to_unset_map.astype(np.int64) > r2)


def dilate(mask, r2, weights=(1, 1, 1)):
    return dilate_of(distance_map(mask, weights, TO_SET), r2)


def erode(mask, r2, weights=(1, 1, 1)):
    return erode_of(distance_map(mask, weights, TO_UNSET), r2)


def ball(mask, op, r2, weights=(1, 1, 1)):
    if op == DILATE:
        return dilate(mask, r2, weights)
    if op == ERODE:
        return erode(mask, r2, weights)
    if op == OPEN:
        return dilate(erode(mask, r2, weights), r2, weights)
    if op == CLOSE:
        return erode(dilate(mask, r2, weights), r2, weights)
    raise ValueError(op)


def select(dmap, lo2, hi2):
    return (dmap >= lo2) & (dmap <= hi2)


def dmax(dmap, mask=None):
    """(max_d2, first_index, status): over the voxels of the mask (None = all) whose value is not NONE; the smallest index on a tie."""
    flat = dmap.reshape(-1).astype(np.int64)
    ok = flat != NONE
    if mask is not None:
        ok &= mask.reshape(-1)
    if not ok.any():
        return 0, 0, rr.EMPTY
    m = int(flat[ok].max())
    return m, int(np.flatnonzero(ok & (flat == m))[0]), rr.OK


def to_volume(dmap, scale):
    out = np.empty(dmap.shape, dtype=np.uint16)
    flat, o = dmap.reshape(-1), out.reshape(-1)
    for i, v in enumerate(flat.tolist()):
        o[i] = 65535 if v == NONE else min(65535, math.isqrt(v * scale * scale))
    return out


def _llround(x):
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def weights(spacing, shape):
    """((wx, wy, wz), unit, k) by the definition of svr_region_distance_weights; ValueError where the call refuses."""
    sp = [float(s) for s in spacing]
    if not all(s > 0.0 and math.isfinite(s) for s in sp):
        raise ValueError("spacing")
    for k in (4, 3, 2, 1, 0):
        unit = min(sp) / float(1 << k)
        if not unit > 0.0:
            continue
        w = []
        for s in sp:
            r = s / unit
            w.append(max(1, _llround(r * r)))
        if all(t <= NONE for t in w) and fits(w, shape):
            return tuple(w), unit, k
    raise ValueError("no k fits")


# ---------------------------------------------------------------------------------------------- fixtures shared by the CPU and GPU tests
WEIGHTS = ((1, 1, 1), (1, 4, 9), (49, 49, 225))
DENSITIES = (0.02, 0.3, 0.9)
BALL_R2 = (0, 1, 2, 3, 4, 9, 50)


def random_mask(shape, density, seed=5):
    return np.random.default_rng(seed).random(shape) < density


def single_map(shape, zyx, weights_, target):
    """The map of a mask with the single voxel `zyx` set, in closed form: TO_SET is the weighted squared distance to it; TO_UNSET is 0
    everywhere but at the voxel itself, whose nearest unset voxel is its cheapest neighbour inside the volume (none in a 1 x 1 x 1 volume)."""
    nz, ny, nx = shape
    z, y, x = np.ogrid[:nz, :ny, :nx]
    if target == TO_SET:
        return (weights_[0] * (x - zyx[2]) ** 2 + weights_[1] * (y - zyx[1]) ** 2 + weights_[2] * (z - zyx[0]) ** 2).astype(np.uint32)
    out = np.zeros(shape, dtype=np.uint32)
    near = [w for w, n in zip(weights_, (nx, ny, nz)) if n > 1]
    out[zyx] = min(near) if near else NONE
    return out


def corners(shape):
    nz, ny, nx = shape
    return sorted({(z, y, x) for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)})


def single(shape, zyx):
    m = np.zeros(shape, dtype=bool)
    m[zyx] = True
    return m


def beyond(weights_, shape):
    """An r2 above every distance in the volume."""
    nz, ny, nx = shape
    return weights_[0] * (nx - 1) ** 2 + weights_[1] * (ny - 1) ** 2 + weights_[2] * (nz - 1) ** 2 + 1


# whole rows and whole slices without a target: the SVR_DIST_NONE sites of the column passes
def sparse_cases():
    a = np.zeros((300, 8, 8), dtype=bool)
    a[0] = True
    b = np.zeros((17, 16, 256), dtype=bool)
    b[0, 0, :] = True
    c = np.zeros((1, 1, 256), dtype=bool)
    c[0, 0, 255] = True
    return [("slice0", a), ("row0", b), ("x255", c)]


LONG_SHAPES = [(1, 1, 2048), (1, 2048, 2), (2048, 2, 1)]


def long_masks(shape):
    """Targets only at the two ends of the long axis, and a target every 37th voxel."""
    n = int(np.prod(shape))
    ends = np.zeros(n, dtype=bool)
    ends[0] = ends[-1] = True
    every = np.zeros(n, dtype=bool)
    every[::37] = True
    return [("ends", ends.reshape(shape)), ("every37", every.reshape(shape))]


# one block of a column pass covers DISTANCE_COLUMN_BLOCK columns (lanes, 32 per mask word of a row): the y pass of this shape has
# nz * wx * 32 = 9 * 32 = 288 lanes and the z pass ny * wx * 32 = 288 -- two blocks each, the second partly filled
BLOCK_SHAPE = (9, 9, 3)

# the maximum of the TO_UNSET map is attained twice: two 3 x 3 x 3 cubes whose centres (z, y, x) = (2, 2, 2) and (2, 2, 7) are the only
# voxels at squared distance 4 from the background; the first in index order is (2 * 6 + 2) * 11 + 2 = 156
TIE_SHAPE = (5, 6, 11)
TIE_INDEX = 156
TIE_D2 = 4


def tie_mask():
    m = np.zeros(TIE_SHAPE, dtype=bool)
    m[1:4, 1:4, 1:4] = True
    m[1:4, 1:4, 6:9] = True
    return m


def cached(key, make):
    return rr.cached(("distance",) + tuple(key), make)


def cached_map(name, mask, weights_=(1, 1, 1), target=TO_SET):
    """One reference map per named case for the whole session."""
    return cached((name, mask.shape, tuple(weights_), target), lambda: distance_map(mask, weights_, target))
