"""Test-side reference of the crop / resample calls (include/svr_abi.h): a literal transcription of the definitions in
numpy int64 and Python ints.  A grid is ((origin, step, count) of x, of y, of z) in Q16 source edge coordinates; volumes are [nz][ny][nx]."""
import math

import numpy as np

NEAREST, LINEAR, AREA, AUTO = 0, 1, 2, 3
MODES = (NEAREST, LINEAR, AREA, AUTO)
MIN_STEP, MAX_STEP = 1024, 4194304
ONE = 65536
PASTE_REPLACE, MASK_OR, MASK_ANDNOT = 0, 2, 3


class Refused(Exception):
    def __init__(self, code, why=""):
        super().__init__(f"{code}: {why}")
        self.code = code


def is_copy(axis_map) -> bool:
    origin, step, _ = axis_map
    return step == ONE and origin % ONE == 0


# ---------------------------------------------------------------- the per-axis definitions
def axis_nearest(v: np.ndarray, axis: int, origin: int, step: int, count: int) -> np.ndarray:
    n = v.shape[axis]
    j = np.arange(count, dtype=np.int64)
    c = origin + j * step + (step >> 1)
    return np.take(v, np.clip(c >> 16, 0, n - 1), axis=axis)


def axis_linear(v: np.ndarray, axis: int, origin: int, step: int, count: int) -> np.ndarray:
    n = v.shape[axis]
    j = np.arange(count, dtype=np.int64)
    t = origin + j * step + (step >> 1) - 32768
    i, f = t >> 16, t & 65535
    shape = [1, 1, 1]
    shape[axis] = count
    f = f.reshape(shape)
    lo = np.take(v, np.clip(i, 0, n - 1), axis=axis).astype(np.int64)
    hi = np.take(v, np.clip(i + 1, 0, n - 1), axis=axis).astype(np.int64)
    acc = lo * (ONE - f) + hi * f + 32768
    assert int(acc.max()) < 1 << 32
    return (acc >> 16).astype(np.uint16)


def axis_area(v: np.ndarray, axis: int, origin: int, step: int, count: int) -> np.ndarray:
    n = v.shape[axis]
    outs = []
    for j in range(count):
        a = origin + j * step
        s = np.zeros(np.take(v, 0, axis=axis).shape, dtype=np.int64)
        total = 0
        for i in range(a >> 16, ((a + step - 1) >> 16) + 1):
            ov = min(a + step, (i + 1) << 16) - max(a, i << 16)
            total += ov
            s += np.take(v, min(max(i, 0), n - 1), axis=axis).astype(np.int64) * ov
        assert total == step
        outs.append(((2 * s + step) // (2 * step)).astype(np.uint16))
    return np.stack(outs, axis=axis)


def axis_mode(mode: int, step: int) -> int:
    return mode if mode != AUTO else (LINEAR if step <= ONE else AREA)


def volume_resample(vol: np.ndarray, grid, mode: int) -> np.ndarray:
    """Passes in the order x, y, z, one rounding per axis."""
    assert vol.dtype == np.uint16 and vol.ndim == 3
    fn = {NEAREST: axis_nearest, LINEAR: axis_linear, AREA: axis_area}
    for a, (origin, step, count) in enumerate(grid):
        vol = fn[axis_mode(mode, step)](vol, 2 - a, int(origin), int(step), int(count))
    return np.ascontiguousarray(vol)


def nearest_any(arr: np.ndarray, grid) -> np.ndarray:
    """NEAREST on an array of any dtype: bool masks and uint32 maps."""
    for a, (origin, step, count) in enumerate(grid):
        arr = axis_nearest(arr, 2 - a, int(origin), int(step), int(count))
    return np.ascontiguousarray(arr)


def paste(full: np.ndarray, sub: np.ndarray, offset_xyz, op: int) -> np.ndarray:
    ox, oy, oz = offset_xyz
    nz, ny, nx = sub.shape
    out = full.copy()
    box = out[oz:oz + nz, oy:oy + ny, ox:ox + nx]
    assert box.shape == sub.shape
    if op == PASTE_REPLACE:
        box[...] = sub
    elif op == MASK_OR:
        box |= sub
    else:
        assert op == MASK_ANDNOT
        box &= ~sub
    return out


def expand(mask: np.ndarray, value: int) -> np.ndarray:
    return np.where(mask, np.uint8(value), np.uint8(0)).astype(np.uint8)


# ---------------------------------------------------------------- the grid helpers
def clamp_box(dims, box_min, box_max):
    b0, b1 = [], []
    for a in range(3):
        lo = 0 if box_min is None else box_min[a]
        hi = dims[a] - 1 if box_max is None else box_max[a]
        if lo > hi or hi < 0 or lo >= dims[a]:
            raise Refused(-3, "box")
        b0.append(max(lo, 0))
        b1.append(min(hi, dims[a] - 1))
    return b0, b1


def check_grid(dims, grid):
    for a, (origin, step, count) in enumerate(grid):
        if not MIN_STEP <= step <= MAX_STEP:
            raise Refused(-3, "step")
        if count == 0 or abs(origin) >= 1 << 47:
            raise Refused(-3, "count / origin")
        if origin + count * step <= 0 or origin >= dims[a] << 16:
            raise Refused(-3, "extent")


def grid_box(dims, box_min, box_max):
    b0, b1 = clamp_box(dims, box_min, box_max)
    return tuple((b0[a] << 16, ONE, b1[a] - b0[a] + 1) for a in range(3))


def grid_spacing(dims, src_spacing, target_spacing, box_min=None, box_max=None):
    """(grid, spacing applied)"""
    b0, b1 = clamp_box(dims, box_min, box_max)
    grid = []
    for a in range(3):
        step = int(math.floor(65536.0 * target_spacing[a] / src_spacing[a] + 0.5))      # llround of a positive number
        if not MIN_STEP <= step <= MAX_STEP:
            raise Refused(-3, "step")
        grid.append((b0[a] << 16, step, max(1, ((b1[a] - b0[a] + 1) * ONE + (step >> 1)) // step)))
    check_grid(dims, grid)
    return tuple(grid), tuple(src_spacing[a] * grid[a][1] / 65536.0 for a in range(3))


def grid_dims(dims, out_dims, box_min=None, box_max=None):
    b0, b1 = clamp_box(dims, box_min, box_max)
    grid = []
    for a in range(3):
        step = ((b1[a] - b0[a] + 1) * ONE + out_dims[a] // 2) // out_dims[a]
        if not MIN_STEP <= step <= MAX_STEP:
            raise Refused(-3, "step")
        grid.append((b0[a] << 16, step, out_dims[a]))
    check_grid(dims, grid)
    return tuple(grid)


def grid_shape(grid):
    """(nz, ny, nx) of the output"""
    return (grid[2][2], grid[1][2], grid[0][2])
