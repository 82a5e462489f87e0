"""A literal numpy reference of the fill-between-slices calls (include/svr_abi.h, "fill between slices"): the set voxels of
every slice, the planar maps by brute force over the voxels of a slice (no separable trick), and the fill rule in uint64.  Masks are bool
arrays [nz][ny][nx]; axis is 0, 1, 2 = x, y, z, so slice k of an axis is np.take(mask, k, axis=2 - axis), an array [nv][nu] with the
lower in-plane axis u fastest."""
import numpy as np

NONE = 0xFFFFFFFF


def planes(mask, axis):
    """The slices of an axis as one array [n_axis][nv][nu] (a view where numpy can make one)."""
    return np.moveaxis(mask, 2 - axis, 0)


def planar_weights(axis, weights=None):
    """(wu, wv) of the weights (wx, wy, wz); None = 1, 1, 1"""
    w = (1, 1, 1) if weights is None else tuple(int(t) for t in weights)
    u, v = [a for a in range(3) if a != axis]
    return w[u], w[v]


def slice_counts(mask, axis):
    """The set voxels of every slice of the axis: uint64[n_axis]"""
    return planes(mask, axis).reshape(mask.shape[2 - axis], -1).sum(axis=1).astype(np.uint64)


def planar_map(s, wu=1, wv=1):
    """The planar map of one slice s (bool [nv][nu]): for every voxel the smallest wu du^2 + wv dv^2 to a voxel of the other kind, NONE
    where the slice holds none.  Brute force: every voxel against every voxel of the other kind."""
    nv, nu = s.shape
    out = np.full((nv, nu), NONE, dtype=np.uint64)
    vv, uu = np.nonzero(np.ones_like(s))
    vv, uu = vv.astype(np.int64), uu.astype(np.int64)
    flat = s.reshape(-1)
    for kind in (False, True):
        mine, other = np.nonzero(flat == kind)[0], np.nonzero(flat != kind)[0]
        if len(mine) == 0 or len(other) == 0:
            continue
        best = np.full(len(mine), NONE, dtype=np.int64)
        for c0 in range(0, len(other), 4096):                       # (in chunks: the table of all pairs need not fit)
            o = other[c0:c0 + 4096]
            d2 = wu * (uu[mine][:, None] - uu[o][None, :]) ** 2 + wv * (vv[mine][:, None] - vv[o][None, :]) ** 2
            best = np.minimum(best, d2.min(axis=1))
        out.reshape(-1)[mine] = best.astype(np.uint64)
    return out.astype(np.uint32)


def slice_distance(mask, axis, weights=None, slices=None):
    """The planar maps of the listed slices (None = all, in order): uint32 [len(slices)][nv][nu]"""
    wu, wv = planar_weights(axis, weights)
    p = planes(mask, axis)
    ks = range(p.shape[0]) if slices is None else [int(k) for k in slices]
    return np.stack([planar_map(p[k], wu, wv) for k in ks]) if len(ks) else np.zeros((0,) + p.shape[1:], dtype=np.uint32)


def auto_keys(mask, axis):
    return [int(k) for k in np.nonzero(slice_counts(mask, axis))[0]]


def fill_between(mask, axis=2, keys=None, weights=None, keep_between=False):
    """(the filled mask, info) -- info: a dict of keys, gaps, filled_slices, first_key, last_key, voxels_in, voxels_out"""
    wu, wv = planar_weights(axis, weights)
    keys = auto_keys(mask, axis) if keys is None else [int(k) for k in keys]
    src = planes(mask, axis)
    out = src.copy()
    gaps = filled = 0
    for a, b in zip(keys[:-1], keys[1:]):
        n = b - a
        if n < 2:
            continue
        gaps, filled = gaps + 1, filled + n - 1
        sa, sb = src[a], src[b]
        A, B = planar_map(sa, wu, wv).astype(np.uint64), planar_map(sb, wu, wv).astype(np.uint64)
        for k in range(a + 1, b):
            t = k - a
            pa, pb = np.uint64((n - t) ** 2) * A, np.uint64(t ** 2) * B          # below 2^64: n <= 65535, the maps below 2^32
            r = (sa & sb) | (sa & ~sb & (pa > pb)) | (sb & ~sa & (pb > pa))
            out[k] = (r | src[k]) if keep_between else r
    res = np.ascontiguousarray(np.moveaxis(out, 0, 2 - axis))
    info = dict(axis=axis, keys=len(keys), gaps=gaps, filled_slices=filled, first_key=keys[0] if keys else -1, last_key=keys[-1] if keys else -1,
                voxels_in=int(mask.sum()), voxels_out=int(res.sum()))
    return res, info


def dice(a, b):
    both, na, nb = int((a & b).sum()), int(a.sum()), int(b.sum())
    return 2.0 * both / (na + nb) if na + nb else float("nan")
