"""Test-side reference of the mask calls (include/svr_abi.h, "operations on region masks"), numpy only and literal: dilate and erode are
ORs / ANDs of shifted arrays with the border rules of the contract (nothing enters a dilation from outside; outside counts as set for an
erosion), reconstruct iterates r |= dilate(r) & cand to the fixpoint, and fill and detach are composed from those.  Nothing here knows
about words, tiles or sweeps.  Masks are bool arrays [nz][ny][nx]."""
import numpy as np

from tests import region_ref as rr

DILATE, ERODE, OPEN, CLOSE = 1, 2, 3, 4
AND, OR, ANDNOT, XOR, NOT = 1, 2, 3, 4, 5
MAX_RADIUS = 32
ELEMENTS = (6, 18, 26)
OPS = (DILATE, ERODE, OPEN, CLOSE)


def dilate1(m, element):
    out = m.copy()
    for o in rr.offsets(element):
        out |= rr.shifted(m, o)                          # (False moves in from outside)
    return out


def erode1(m, element):
    return ~dilate1(~m, element)                         # the dual: a voxel outside the volume counts as set


def dilate(m, element, radius=1):
    for _ in range(radius):
        m = dilate1(m, element)
    return m


def erode(m, element, radius=1):
    for _ in range(radius):
        m = erode1(m, element)
    return m


def morph(m, op, element, radius=1):
    if op == DILATE:
        return dilate(m, element, radius)
    if op == ERODE:
        return erode(m, element, radius)
    if op == OPEN:
        return dilate(erode(m, element, radius), element, radius)
    if op == CLOSE:
        return erode(dilate(m, element, radius), element, radius)
    raise ValueError(op)


def combine(a, b, op):
    return {AND: lambda: a & b, OR: lambda: a | b, ANDNOT: lambda: a & ~b, XOR: lambda: a ^ b, NOT: lambda: ~a}[op]()


def reconstruct(marker, cand, connectivity=6):
    r = marker & cand
    while True:
        n = (r | dilate1(r, connectivity)) & cand
        if np.array_equal(n, r):
            return r
        r = n


def faces(shape):
    f = np.zeros(shape, dtype=bool)
    f[0] = f[-1] = True
    f[:, 0] = f[:, -1] = True
    f[:, :, 0] = f[:, :, -1] = True
    return f


def fill_holes(m, background_connectivity=6):
    return ~reconstruct(faces(m.shape), ~m, background_connectivity)


def points(shape, seeds):
    p = np.zeros(shape, dtype=bool)
    for x, y, z in seeds:
        p[z, y, x] = True
    return p


def detach(m, seeds, element=6, radius=1, connectivity=6):
    """(mask, status)"""
    core = erode(m, element, radius)
    k = reconstruct(dilate(points(m.shape, seeds), element, radius), core, connectivity)
    out = dilate(k, element, radius) & m
    return out, (rr.OK if out.any() else rr.EMPTY)


# ---------------------------------------------------------------------------------------------- fixtures shared by the CPU and GPU tests
def random_mask(shape, density, seed=5):
    return np.random.default_rng(seed).random(shape) < density


def dirty_padding(words, shape, fill=0xFFFFFFFF):
    """The words of a mask with the padding bits (x >= nx of a row's last word) replaced by those of `fill`."""
    nz, ny, nx = shape
    wx = (nx + 31) // 32
    w = np.array(words, dtype=np.uint32).reshape(nz, ny, wx)
    if nx % 32:
        pad = np.uint32((0xFFFFFFFF << (nx % 32)) & 0xFFFFFFFF)
        w[:, :, -1] = (w[:, :, -1] & ~pad) | (np.uint32(fill) & pad)
    return w.reshape(-1)


TWO_BALL_SHAPE = (20, 20, 72)
TWO_BALL_SEED = (23, 9, 9)


def two_balls():
    """Two balls of radius 6 at x = 20 and x = 50 (y = z = 9) joined by a bridge one voxel wide along y = z = 9, the first with a hole of 19
    voxels at its centre: 1848 voxels.  Crosses the word boundaries at x = 32 and 64 and the tile boundaries at y = z = 8."""
    z, y, x = np.ogrid[:20, :20, :72]
    r1 = (x - 20) ** 2 + (y - 9) ** 2 + (z - 9) ** 2
    r2 = (x - 50) ** 2 + (y - 9) ** 2 + (z - 9) ** 2
    m = (r1 <= 36) | (r2 <= 36)
    m[9, 9, 20:51] = True
    m &= ~(r1 <= 2)
    return m


def second_ball(mask):
    return int(mask[:, :, 44:].sum())


def serpentine_mask():
    vox, seed = rr.serpentine()
    return vox == 1000, seed


def cached(key, make):
    return rr.cached(("morph",) + tuple(key), make)
