"""numpy restatement of adaptive sampling (include/svr_abi.h, svr_render_pathtracer_adaptive): the checkpoints, the freeze rule and the final
tile RMSE, replayed from the tile estimates of uniform renders (tests/noise_ref.py).  A tile's pixels are a pure function of its frame count,
and all active tiles share one (m, n), so the estimate an adaptive call makes for an active tile is the uniform render's."""
from __future__ import annotations

import numpy as np

TILE = 16


def schedule(f0: int, max_frames: int) -> list:
    """Frame counts of the call's checkpoints within f0 + max_frames: the snapshot max(f0 + 1, 4), then the estimates at n = 2m."""
    end = f0 + max_frames
    pts, n = [], max(f0 + 1, 4)
    while n <= end:
        pts.append(n)
        n *= 2
    return pts


def tile_pixels(H: int, W: int) -> np.ndarray:
    """Pixels of each 16 x 16 tile, (ceil(H/16), ceil(W/16))."""
    ty, tx = -(-H // TILE), -(-W // TILE)
    h = np.minimum(TILE, H - TILE * np.arange(ty))
    w = np.minimum(TILE, W - TILE * np.arange(tx))
    return np.outer(h, w).astype(np.int64)


def replay(f0: int, min_frames: int, max_frames: int, target: float, estimate, shape) -> dict:
    """The call's decisions.  estimate(m, n) -> (tile RMSE, counted pixels per tile), maps of `shape` = (tiles_y, tiles_x), for the estimate
    at n against the snapshot at m.  Returns the tile frame counts, the final tile RMSE (the last estimate scaled by sqrt(n_est / n_final)),
    sse / pixels / rmse / tile_max, the checkpoint count and the active tiles at the end."""
    end = f0 + max_frames
    pts = schedule(f0, max_frames)
    frames = np.full(shape, f0, np.int64)
    active = np.ones(shape, bool)
    prev = np.zeros(shape, bool)
    rmse = np.full(shape, np.nan)
    cnt = np.zeros(shape, np.int64)
    est_n = np.zeros(shape, np.int64)
    checkpoints = 0
    done = False
    for i, n in enumerate(pts):
        frames[active] = n
        if i == 0:
            continue
        r, c = estimate(pts[i - 1], n)
        r, c = np.asarray(r, np.float64), np.asarray(c, np.int64)
        checkpoints += 1
        rmse[active], cnt[active], est_n[active] = r[active], c[active], n
        with np.errstate(invalid="ignore"):
            below = ~(r > target)                     # a NaN tile (no counted pixel) counts as below
        freeze = active & below & prev & (n >= min_frames)
        prev = np.where(active, below, prev)
        active &= ~freeze
        if not active.any():
            done = True
            break
    if not done:
        frames[active] = end
    has = (est_n > 0) & (cnt > 0)
    scale = np.where(est_n > 0, est_n / np.maximum(frames, 1), 0.0)
    final = np.where(has, rmse * np.sqrt(scale), np.nan)
    sse = float(np.sum(np.where(has, rmse ** 2 * cnt * scale, 0.0)))
    pixels = int(cnt[est_n > 0].sum())
    return {"frames": frames, "tile_rmse": final, "sse": sse, "pixels": pixels, "rmse": np.sqrt(sse / pixels) if pixels else np.nan,
            "tile_max": float(np.nanmax(final)) if has.any() else np.nan, "checkpoints": checkpoints, "active": active,
            "frames_max": int(frames.max()), "frames_min": int(frames.min())}


def pixel_frames(frames: np.ndarray, f0: int, H: int, W: int) -> int:
    """Samples traced by the call: sum over tiles of pixels(t) * (frames_t - f0)."""
    return int(np.sum(tile_pixels(H, W) * (np.asarray(frames, np.int64) - f0)))
