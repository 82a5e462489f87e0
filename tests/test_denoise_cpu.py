"""Denoised preview, host side: the svr_denoise_params layout and defaults, and the numpy restatement of the filter on a
synthetic case (no GPU)."""
import ctypes as C

import numpy as np

from sunvolumerender_amd import abi
from tests.denoise_ref import atrous_ref


def test_params_layout_and_option_key():
    P = abi.DenoiseParams
    assert C.sizeof(P) == 28
    assert [getattr(P, f).offset for f in ("passes", "sigma_depth", "sigma_normal", "sigma_albedo", "sigma_opacity", "sigma_color", "step")] == \
        [0, 4, 8, 12, 16, 20, 24]
    assert abi.OPT_DENOISE_PREVIEW == 36
    for name in ("svr_denoise_params_default", "svr_set_denoise_params", "svr_render_guides", "svr_denoise_to_ldr", "svr_denoise_hdr"):
        assert name in abi.PROTOTYPES


def test_params_defaults_from_the_library():
    lib = abi.load()                              # no GPU needed: the defaults are plain host code
    p = abi.DenoiseParams()
    assert lib.svr_denoise_params_default(C.byref(p)) == 0
    assert p.passes == 5 and p.sigma_color == 0.0 and p.step == 0.0
    assert p.sigma_depth > 0 and p.sigma_normal > 0 and p.sigma_albedo > 0 and p.sigma_opacity > 0


def _synthetic(H=40, W=48, seed=3):
    """Two flat slabs (different depth, normal, albedo) on a background with O == 0, plus per-pixel noise."""
    rng = np.random.default_rng(seed)
    g = np.zeros((H, W, 8), dtype=np.float32)
    g[..., 3], g[..., 4:7], g[..., 7] = -1.0, 1.0, 0.0            # background sentinels
    g[5:35, 4:24, 0:3] = (0.0, 0.0, 1.0)
    g[5:35, 4:24, 3] = 10.0
    g[5:35, 4:24, 4:7] = (0.8, 0.5, 0.3)
    g[5:35, 4:24, 7] = 1.0
    g[5:35, 24:44, 0:3] = (0.0, 1.0, 0.0)
    g[5:35, 24:44, 3] = 20.0
    g[5:35, 24:44, 4:7] = (0.2, 0.4, 0.9)
    g[5:35, 24:44, 7] = 0.9
    clean = np.where(g[..., 7:8] > 0, g[..., 4:7] * 0.5, 0.25).astype(np.float32)
    noisy = (clean * rng.exponential(1.0, clean.shape)).astype(np.float32)
    return g, clean, noisy


def test_reference_filter_denoises_and_keeps_edges():
    g, clean, noisy = _synthetic()
    out = atrous_ref(noisy, g, pix_scale=0.01)
    fg = g[..., 7] > 0
    # pass-through: O == 0 pixels are returned untouched
    assert np.array_equal(out[~fg], noisy[~fg].astype(np.float64))
    # less noise inside the slabs, and no bleeding across the depth / albedo edge between them
    err_in = np.sqrt(np.mean((noisy[fg] - clean[fg]) ** 2))
    err_out = np.sqrt(np.mean((out[fg] - clean[fg]) ** 2))
    assert err_out < 0.5 * err_in, (err_out, err_in)
    left, right = out[5:35, 20:24], out[5:35, 24:28]
    assert abs(left[..., 2].mean() / right[..., 2].mean() - (0.3 / 0.9)) < 0.1


def test_reference_filter_properties():
    g, clean, noisy = _synthetic()
    # a constant signal per slab is a fixed point (weights are normalised per pixel)
    out = atrous_ref(clean, g, pix_scale=0.01)
    assert np.allclose(out, clean, rtol=1e-12, atol=0)
    # zero passes is the identity; the colour term only ever reduces smoothing
    assert np.allclose(atrous_ref(noisy, g, passes=0), noisy, rtol=1e-12, atol=0)
    a = atrous_ref(noisy, g, pix_scale=0.01)
    b = atrous_ref(noisy, g, pix_scale=0.01, sigma_color=0.05)
    fg = g[..., 7] > 0
    assert np.std(b[fg] - clean[fg]) >= np.std(a[fg] - clean[fg])
    # deterministic
    assert np.array_equal(a, atrous_ref(noisy, g, pix_scale=0.01))
