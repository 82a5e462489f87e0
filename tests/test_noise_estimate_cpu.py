"""Noise estimate, host side (no GPU): the svr_noise_estimate layout against the header, the option key, the new symbols, the `-noise`
argument of examples/render_mhd.cpp, and the estimator's statistics on simulated samples (numpy restatement)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi
from tests.noise_ref import estimate_ref, measured_error
from tests.cpp_example import build_example

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()


def test_struct_layout_matches_header():
    E = abi.NoiseEstimate
    assert C.sizeof(E) == 48
    names = ["frames", "frames_ref", "rmse", "tile_max", "tiles_x", "tiles_y", "pixels", "nonfinite", "sse"]
    assert [f for f, _ in E._fields_] == names
    assert [getattr(E, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 32, 40]
    body = re.search(r"typedef struct svr_noise_estimate \{(.*?)\} svr_noise_estimate;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(uint32_t|uint64_t|float|double)\s+([a-z_, ]+);", body)
    fields = [(t, n.strip()) for t, ns in decl for n in ns.split(",")]
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
    assert [n for _, n in fields] == names
    assert [ctype[t] for t, _ in fields] == [t for _, t in E._fields_]


def test_option_key_and_symbols():
    assert abi.OPT_NOISE_ESTIMATE == 37
    assert re.search(r"#define SVR_OPT_NOISE_ESTIMATE 37\b", HEADER)
    lib = C.CDLL(str(abi.library_path()))
    for name in ("svr_get_noise_estimate", "svr_estimate_noise", "svr_render_pathtracer_until"):
        assert name in abi.PROTOTYPES and hasattr(lib, name), name


@pytest.fixture(scope="module")
def render_mhd(tmp_path_factory):
    exe = build_example(tmp_path_factory.mktemp("render_mhd"), strict=True)
    return exe


@pytest.mark.parametrize("value", ["abc", "0", "-0.01", "nan", "0.01x"])
def test_render_mhd_rejects_bad_noise_target(render_mhd, tmp_path, value):
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), "-noise", value], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2, res.stdout + res.stderr
    assert "-noise needs a target RMSE > 0" in res.stderr


def test_render_mhd_accepts_noise_target(render_mhd, tmp_path):
    # parsed: the program goes on to the device / the volume (which does not exist) and fails there, not on its arguments
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), "-noise", "0.005", "-frames", "256"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode not in (0, 2), res.stdout + res.stderr
    assert "unknown argument" not in res.stderr and "-noise needs" not in res.stderr
    assert "-noise T" in subprocess.run([str(render_mhd)], capture_output=True, text=True, timeout=60).stderr


def test_reference_estimator_is_calibrated_on_simulated_samples():
    """Independent samples per pixel with heavy-ish tails: the predicted RMSE at n = 2m (and n = 3m) against the known mean matches the
    measured tone-mapped RMSE of A(n), and the tile map ranks the tiles by their noise."""
    rng = np.random.default_rng(11)
    H, W, n = 48, 64, 256
    mean = np.zeros((H, W, 3))
    mean[..., 0] = np.linspace(0.005, 0.08, W)[None, :]
    mean[..., 1] = np.linspace(0.01, 0.06, H)[:, None]
    mean[..., 2] = 0.03
    cv = np.repeat(np.linspace(0.3, 3.0, W)[None, :], H, axis=0)[..., None]        # per-pixel coefficient of variation
    shape = 1.0 / cv ** 2
    samples = rng.gamma(shape[None], (mean / shape)[None], size=(n, H, W, 3))
    acc = np.cumsum(samples, axis=0) / np.arange(1, n + 1)[:, None, None, None]
    exposure = 1.3
    for m, nn in ((64, 128), (64, 192), (128, 256)):
        est = estimate_ref(acc[m - 1], m, acc[nn - 1], nn, exposure)
        e2, ok = measured_error(acc[nn - 1], mean, exposure)
        meas = np.sqrt(e2[ok].mean())
        assert est["pixels"] == H * W and est["nonfinite"] == 0
        assert 0.85 <= est["rmse"] / meas <= 1.15, (m, nn, est["rmse"], meas)
        # noisier columns -> larger tile RMSE, left to right
        t = est["tiles"]
        assert np.all(np.diff(t.mean(axis=0)) > 0), t


def test_reference_estimator_counts():
    a = np.full((20, 35, 3), 0.05, np.float32)
    b = a * 1.1
    a[0, 9, 1] = np.nan
    b[3, 12, 0] = np.inf
    b[19, 34, 2] = -np.inf
    a[5, 2, 0] = np.nan                   # not owned: neither counted nor non-finite
    own = np.ones((20, 35), bool)
    own[:, :8] = False
    r = estimate_ref(a, 4, b, 8, 1.0, owned=own)
    assert r["nonfinite"] == 3 and r["pixels"] == 20 * 27 - 3
    assert r["tiles"].shape == (2, 3) and np.isfinite(r["tiles"]).all()
    r = estimate_ref(a, 4, b, 8, 1.0, owned=np.zeros((20, 35), bool))
    assert r["pixels"] == 0 and np.isnan(r["rmse"]) and np.isnan(r["tiles"]).all() and np.isnan(r["tile_max"])
