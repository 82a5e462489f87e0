"""numpy reference of the smoothing calls (include/svr_abi.h, "smoothing region masks and label maps"): the box count by
edge padding and separable cumulative sums, MAJORITY from it, BINOMIAL through tests/filter_ref.py's smoothing reference, MODE by the
per-class loop with the tie rule.  Arrays are [nz][ny][nx]; radii are (rx, ry, rz)."""
import numpy as np

from tests import filter_ref

MAJORITY, BINOMIAL = 1, 2


def box_size(radii) -> int:
    rx, ry, rz = radii
    return (2 * rx + 1) * (2 * ry + 1) * (2 * rz + 1)


def box_sum(a: np.ndarray, radii) -> np.ndarray:
    """the sum of the window around every voxel, the border replicated (int64)"""
    out = a.astype(np.int64)
    for axis, r in zip((2, 1, 0), radii):
        if r == 0:
            continue
        pad = [(0, 0)] * 3
        pad[axis] = (r + 1, r)
        c = np.cumsum(np.pad(out, pad, mode="edge"), axis=axis)
        n = out.shape[axis]
        out = np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=axis) - np.take(c, np.arange(n), axis=axis)
    return out


def box_count(mask: np.ndarray, radii) -> np.ndarray:
    return box_sum(mask.astype(bool), radii).astype(np.uint16)


def majority(mask: np.ndarray, radii) -> np.ndarray:
    return 2 * box_sum(mask.astype(bool), radii) > box_size(radii)


def binomial(mask: np.ndarray, radii) -> np.ndarray:
    e = np.where(mask, 65535, 0).astype(np.uint16)
    return filter_ref.smooth(e, radii) >= 32768


def smooth(mask: np.ndarray, op: int, radii, iterations: int = 1):
    """(mask, changed)"""
    out = mask.astype(bool)
    for _ in range(iterations):
        out = majority(out, radii) if op == MAJORITY else binomial(out, radii)
    return out, int((out != mask.astype(bool)).sum())


def read_labels(labels: np.ndarray, count: int) -> np.ndarray:
    """the map as the library reads it: a value above count is 0"""
    lab = labels.astype(np.int64)
    return np.where(lab > count, 0, lab)


def mode_once(lab: np.ndarray, count: int, radii) -> np.ndarray:
    best = np.full(lab.shape, -1, np.int64)
    arg = np.zeros(lab.shape, np.int64)
    own = np.zeros(lab.shape, np.int64)
    for label in range(count + 1):
        member = lab == label
        if not member.any():
            continue
        c = box_sum(member, radii)
        take = c > best                                       # strictly: the smallest label keeps a tie
        best, arg = np.where(take, c, best), np.where(take, label, arg)
        own = np.where(member, c, own)
    return np.where(own == best, lab, arg)


def label_smooth(labels: np.ndarray, count: int, radii, iterations: int = 1):
    """(labels as uint32, changed)"""
    first = read_labels(labels, count)
    out = first
    for _ in range(iterations):
        out = mode_once(out, count, radii)
    return out.astype(np.uint32), int((out != first).sum())


def mode_brute(labels: np.ndarray, count: int, radii) -> np.ndarray:
    """one iteration by a bincount per window"""
    rx, ry, rz = radii
    lab = read_labels(labels, count)
    p = np.pad(lab, ((rz, rz), (ry, ry), (rx, rx)), mode="edge")
    out = np.zeros(lab.shape, np.uint32)
    nz, ny, nx = lab.shape
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                c = np.bincount(p[z:z + 2 * rz + 1, y:y + 2 * ry + 1, x:x + 2 * rx + 1].ravel(), minlength=count + 1)
                out[z, y, x] = lab[z, y, x] if c[lab[z, y, x]] == c.max() else int(np.argmax(c))
    return out


def smooth_radii(spacing, size):
    """((rx, ry, rz), (sx, sy, sz)) of svr_region_smooth_radii; halves round away from zero as llround does"""
    r = []
    for s in spacing:
        h = (size / s - 1.0) / 2.0
        r.append(max(0, int(np.floor(h + 0.5))))
    return tuple(r), tuple((2 * t + 1) * s for t, s in zip(r, spacing))


def ball_with_salt(shape, seed=3, salt=0.08):
    """a ball that fills most of the volume with salt-and-pepper noise flipped into it"""
    nz, ny, nx = shape
    z, y, x = np.ogrid[:nz, :ny, :nx]
    m = ((x - nx / 2.0) / max(nx, 2)) ** 2 + ((y - ny / 2.0) / max(ny, 2)) ** 2 + ((z - nz / 2.0) / max(nz, 2)) ** 2 <= 0.16
    return m ^ (np.random.default_rng(seed).random(shape) < salt)
