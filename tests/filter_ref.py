"""The literal numpy reference of the volume filters (svr_volume_rank, svr_volume_smooth; include/svr_abi.h): pad with the edge values,
stack the shifted views of the window, sort, take the rank; per axis an int64 binomial sum, one rounding, one shift.  Nothing here is
fast or clever on purpose.  Volumes are [nz][ny][nx] uint16."""
import functools
import math

import numpy as np

MEDIAN, MIN, MAX = 1, 2, 3
OPS = (MEDIAN, MIN, MAX)
ELEMENTS = (6, 18, 26)
MAX_ITERATIONS, MAX_RADIUS = 64, 8
BONE = (39321, 65535)           # BONE of tests/test_region_cpu.py


def offsets(element: int):
    """The (dz, dy, dx) of the window: the voxel and its neighbours that differ in at most 1 / 2 / 3 coordinates."""
    most = {6: 1, 18: 2, 26: 3}[element]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if abs(dz) + abs(dy) + abs(dx) <= most]


def rank_once(vol: np.ndarray, op: int, element: int) -> np.ndarray:
    assert vol.dtype == np.uint16 and vol.ndim == 3
    nz, ny, nx = vol.shape
    p = np.pad(vol, 1, mode="edge")
    win = np.stack([p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx] for dz, dy, dx in offsets(element)])
    win = np.sort(win, axis=0)
    return np.ascontiguousarray(win[{MEDIAN: len(win) // 2, MIN: 0, MAX: len(win) - 1}[op]])


def rank(vol: np.ndarray, op: int, element: int = 6, iterations: int = 1) -> np.ndarray:
    assert 1 <= iterations <= MAX_ITERATIONS
    for _ in range(iterations):
        vol = rank_once(vol, op, element)
    return vol


def smooth_axis(vol: np.ndarray, axis: int, r: int) -> np.ndarray:
    """One binomial pass of radius r along numpy axis `axis`."""
    assert 0 <= r <= MAX_RADIUS
    if r == 0:
        return vol.copy()
    n = vol.shape[axis]
    pad = [(0, 0)] * 3
    pad[axis] = (r, r)
    p = np.pad(vol, pad, mode="edge").astype(np.int64)
    acc = np.full(vol.shape, 1 << (2 * r - 1), dtype=np.int64)
    for k in range(2 * r + 1):
        sl = [slice(None)] * 3
        sl[axis] = slice(k, k + n)
        acc += math.comb(2 * r, k) * p[tuple(sl)]
    assert acc.max() < 2 ** 32
    out = acc >> (2 * r)
    assert out.max() <= 65535
    return out.astype(np.uint16)


def smooth(vol: np.ndarray, radii_xyz) -> np.ndarray:
    """Passes in the order x, y, z; radii_xyz = (rx, ry, rz)."""
    assert vol.dtype == np.uint16 and vol.ndim == 3
    for a, r in enumerate(radii_xyz):
        vol = smooth_axis(vol, 2 - a, int(r))
    return vol


def radii_from_sigma(spacing, sigma):
    """svr_volume_smooth_radii's definition: (radii, sigma applied)."""
    r = [int(math.floor(2.0 * (sigma / s) ** 2 + 0.5)) for s in spacing]
    return tuple(r), tuple(math.sqrt(k / 2.0) * s for k, s in zip(r, spacing))


# ---------------------------------------------------------------- fixtures
def random_volume(shape, seed: int) -> np.ndarray:
    """Full-range u16: values of 32768 and above are ordinary data."""
    return np.random.default_rng(seed).integers(0, 65536, size=shape, dtype=np.uint16)


def extremes_volume(shape, seed: int) -> np.ndarray:
    """Only 0 and 65535."""
    return (np.random.default_rng(seed).integers(0, 2, size=shape, dtype=np.uint16) * np.uint16(65535)).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def heads():
    """(clean, salted): the 48^3 head phantom, and the same with 1 voxel in 64 replaced by 0 or 65535."""
    from sunvolumerender_amd import scenes

    clean = np.ascontiguousarray(scenes.make_ct_head_volume(48), dtype=np.uint16)
    idx = np.arange(48 ** 3, dtype=np.uint32).reshape(48, 48, 48)                        # (z * 48 + y) * 48 + x
    h = scenes.wang_hash_np(idx + np.uint32(0xC0FFEE))
    salted = clean.copy()
    hit = h % np.uint32(64) == 0
    salted[hit] = np.where((h[hit] >> np.uint32(16)) & np.uint32(1), 65535, 0).astype(np.uint16)
    clean.setflags(write=False)
    salted.setflags(write=False)
    return clean, salted


def window(vol: np.ndarray, lohi=BONE) -> np.ndarray:
    return (vol >= lohi[0]) & (vol <= lohi[1])


@functools.lru_cache(maxsize=None)
def cached_rank(name: str, op: int, element: int, iterations: int = 1) -> np.ndarray:
    """The reference result on one of the named fixtures, computed once per process."""
    vol = {"clean": heads()[0], "salted": heads()[1]}[name]
    out = rank(vol, op, element, iterations)
    out.setflags(write=False)
    return out
