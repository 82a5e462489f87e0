"""Test-side reference of the component calls (include/svr_abi.h, "connected components of region masks"), numpy only and literal: every
set voxel starts with its linear index, "take the minimum over yourself and your set neighbours" is iterated with the shifted arrays of
tests/region_ref.py to the fixpoint, and a voxel's label is the rank of its value among the distinct values.  The table, the selection by
size (with its tie rule) and the threshold are computed from their definitions.  Nothing here knows about words, runs or trees."""
import numpy as np

from tests import region_ref as rr

CONNS = (6, 18, 26)
COMPONENT_FIELDS = ("voxels", "first", "bbox_min", "bbox_max", "sum")


def roots(mask, connectivity):
    """int64 [nz][ny][nx]: the smallest linear index of the voxel's component; -1 for background."""
    mask = np.asarray(mask, dtype=bool)
    n = mask.size
    # rr.shifted fills with 0, so the iteration runs on n - index (> 0, larger = smaller index) with 0 for "no voxel": the minimum of the
    # indices is the maximum of these
    val = np.where(mask, n - np.arange(n, dtype=np.int64).reshape(mask.shape), 0)
    offs = rr.offsets(connectivity)
    while True:
        new = val.copy()
        for o in offs:
            np.maximum(new, rr.shifted(val, o), out=new)
        new[~mask] = 0
        if np.array_equal(new, val):
            break
        val = new
    return np.where(mask, n - val, -1)


def label(mask, connectivity):
    """(labels uint32 [nz][ny][nx], K): components numbered 1 .. K by ascending smallest linear index; 0 = background."""
    r = roots(mask, connectivity)
    distinct = np.unique(r[r >= 0])
    labels = np.zeros(r.shape, dtype=np.uint32)
    labels[r >= 0] = np.searchsorted(distinct, r[r >= 0]) + 1
    return labels, int(len(distinct))


def labelled(name, mask, connectivity):
    """(labels, K) of a named case, computed once."""
    return rr.cached(("label", name, mask.shape, connectivity), lambda: label(mask, connectivity))


def table(labels, count, vox=None):
    """svr_region_component[count] as a dict of arrays (bbox_*: [count][3] in x, y, z order); sum is 0 without a volume."""
    nz, ny, nx = labels.shape
    flat = labels.reshape(-1).astype(np.int64)
    on = np.flatnonzero(flat)
    lab = flat[on] - 1
    z, y, x = np.unravel_index(on, labels.shape)
    t = {"voxels": np.bincount(lab, minlength=count).astype(np.uint32), "first": np.full(count, 0xFFFFFFFF, dtype=np.uint32),
         "bbox_min": np.full((count, 3), np.iinfo(np.int32).max, dtype=np.int32), "bbox_max": np.full((count, 3), -1, dtype=np.int32),
         "sum": np.zeros(count, dtype=np.uint64)}
    np.minimum.at(t["first"], lab, on.astype(np.uint32))
    for a, c in enumerate((x, y, z)):
        np.minimum.at(t["bbox_min"][:, a], lab, c.astype(np.int32))
        np.maximum.at(t["bbox_max"][:, a], lab, c.astype(np.int32))
    if vox is not None:
        np.add.at(t["sum"], lab, vox.reshape(-1)[on].astype(np.uint64))
    return t


def kept_labels(sizes, min_voxels, largest_k):
    """The labels (1-based, ascending) of the components with at least min_voxels voxels among the largest_k largest (0 = no limit); ties
    in size go to the lower label."""
    order = sorted(range(1, len(sizes) + 1), key=lambda i: (-int(sizes[i - 1]), i))
    order = [i for i in order if int(sizes[i - 1]) >= min_voxels and int(sizes[i - 1]) > 0]
    if largest_k:
        order = order[:largest_k]
    return sorted(order)


def select(labels, keep):
    """The mask of the voxels whose label has a non-zero entry in keep (indexed by label; entry 0 is ignored)."""
    k = np.asarray(keep).astype(bool).copy()
    k[0] = False
    return k[labels]


def select_by_size(labels, count, min_voxels, largest_k):
    """(mask, kept)."""
    sizes = np.bincount(labels.reshape(-1), minlength=count + 1)[1:]
    kept = kept_labels(sizes, min_voxels, largest_k)
    keep = np.zeros(count + 1, dtype=np.uint8)
    keep[kept] = 1
    return select(labels, keep), len(kept)


def threshold(vox, lo, hi, box=None):
    return rr.candidates(vox, lo, hi, box)


# ---------------------------------------------------------------------------------------------- fixtures shared by the CPU and GPU tests
DENSITIES = (0.02, 0.3, 0.5)
SCAN3_SHAPE = (257, 256, 2)                              # 65 792 mask words: more than a block of blocks of the renumbering scan (256 * 256)
CHECKER_SHAPE = (64, 64, 64)
LAST_LARGEST_SHAPE = (6, 10, 70)


def random_mask(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def checkerboard(shape=CHECKER_SHAPE):
    z, y, x = np.indices(shape)
    return (x + y + z) % 2 == 0


def last_largest():
    """Three components under every connectivity: two single voxels first, then a block that is the largest and starts last."""
    m = np.zeros(LAST_LARGEST_SHAPE, dtype=bool)
    m[0, 0, 0] = True
    m[0, 0, 40] = True
    m[2:5, 3:9, 20:60] = True
    return m
