"""float64 numpy restatement of the noise estimate (include/svr_abi.h, svr_noise_estimate; csrc/svr_noise.hip)."""
from __future__ import annotations

import numpy as np

TILE = 16


def tm(hdr, exposure):
    """The tone curve before quantisation, T(L) = (1 - e^(-16 exposure L))^2.2 per channel, L clamped at 0."""
    L = np.maximum(np.asarray(hdr, np.float64), 0.0)
    return np.clip(1.0 - np.exp(-16.0 * exposure * L), 0.0, None) ** 2.2


def tile_sums(v, H, W):
    """(H, W) -> per 16 x 16 tile sums, (ceil(H/16), ceil(W/16))."""
    ty, tx = -(-H // TILE), -(-W // TILE)
    p = np.zeros((ty * TILE, tx * TILE), np.float64)
    p[:H, :W] = v
    return p.reshape(ty, TILE, tx, TILE).sum(axis=(1, 3))


def estimate_ref(a_m, m, a_n, n, exposure, owned=None):
    """The estimate of A(n) against A(m) (H x W x 3 each) over the pixels of `owned` (bool H x W; None = all)."""
    a_m, a_n = np.asarray(a_m, np.float64), np.asarray(a_n, np.float64)
    H, W = a_m.shape[:2]
    own = np.ones((H, W), bool) if owned is None else owned
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(a_m).all(-1) & np.isfinite(a_n).all(-1)
        cnt = own & fin
        b = np.where(cnt[..., None], a_n + m / (n - m) * (a_n - a_m), 0.0)
        d2 = np.mean((tm(np.where(cnt[..., None], a_m, 0.0), exposure) - tm(b, exposure)) ** 2, axis=-1)
    e2 = np.where(cnt, d2 * m * (n - m) / float(n) ** 2, 0.0)
    s_t, c_t = tile_sums(e2, H, W), tile_sums(cnt.astype(np.float64), H, W)
    with np.errstate(invalid="ignore", divide="ignore"):
        tiles = np.where(c_t > 0, np.sqrt(s_t / np.maximum(c_t, 1)), np.nan)
    sse, pixels = float(e2.sum()), int(cnt.sum())
    return {"sse": sse, "pixels": pixels, "nonfinite": int((own & ~fin).sum()), "tiles": tiles,
            "rmse": np.sqrt(sse / pixels) if pixels else np.nan, "tile_max": float(np.nanmax(tiles)) if (c_t > 0).any() else np.nan}


def measured_error(a_n, ref, exposure, mask=None):
    """Per-pixel squared tone-mapped error of A(n) against a reference (mean over the channels), and the mask of pixels finite in both."""
    a_n, ref = np.asarray(a_n, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(a_n).all(-1) & np.isfinite(ref).all(-1)
    if mask is not None:
        ok &= mask
    with np.errstate(invalid="ignore"):
        e2 = np.mean((tm(np.where(ok[..., None], a_n, 0), exposure) - tm(np.where(ok[..., None], ref, 0), exposure)) ** 2, axis=-1)
    return np.where(ok, e2, 0.0), ok


def spearman(a, b):
    """Spearman rank correlation (no ties expected in continuous data)."""
    ra = np.argsort(np.argsort(a)).astype(np.float64)
    rb = np.argsort(np.argsort(b)).astype(np.float64)
    return float(np.corrcoef(ra, rb)[0, 1])
