"""Adaptive sampling, host side (no GPU): the numpy restatement of the freeze rule on known answers, the svr_adaptive_result layout against
the header, the new symbols, and the `-adaptive` argument of examples/render_mhd.cpp."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi
from tests.adaptive_ref import pixel_frames, replay, schedule, tile_pixels
from tests.cpp_example import build_example

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()


def test_schedule():
    assert schedule(0, 4096) == [4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
    assert schedule(0, 100) == [4, 8, 16, 32, 64]
    assert schedule(8, 64) == [9, 18, 36, 72]
    assert schedule(3, 10) == [4, 8]
    assert schedule(0, 3) == []


def _const(values):
    """estimate(m, n) of fixed per-checkpoint maps: values[n] = tile RMSE map; a tile counts 256 pixels, a NaN tile none."""
    return lambda m, n: (np.asarray(values[n], np.float64), np.where(np.isnan(values[n]), 0, 256))


def test_freeze_rule_known_answers():
    T = 0.1
    # tile 0: below from 8 on -> frozen at 16; tile 1: below at 16, 32 -> 32; tile 2: below at 8, above at 16, below at 32, 64 -> 64;
    # tile 3: never below -> max_frames; tile 4: no counted pixel (NaN) -> 16
    seq = {8: [0.05, 0.2, 0.05, 0.5, np.nan], 16: [0.04, 0.09, 0.2, 0.4, np.nan], 32: [0.03, 0.08, 0.09, 0.3, np.nan],
           64: [0.02, 0.07, 0.08, 0.2, np.nan], 128: [0.01, 0.05, 0.06, 0.15, np.nan]}
    seq = {n: np.array([v]) for n, v in seq.items()}
    r = replay(0, 0, 100, T, _const(seq), (1, 5))
    assert r["frames"].tolist() == [[16, 32, 64, 100, 16]]
    assert r["checkpoints"] == 4 and r["active"].tolist() == [[False, False, False, True, False]]
    # final tile RMSE: frozen tiles keep their estimate, the active one is scaled from 64 to 100 frames
    np.testing.assert_allclose(r["tile_rmse"][0, :4], [0.04, 0.08, 0.08, 0.2 * np.sqrt(64 / 100)], rtol=1e-12)
    assert np.isnan(r["tile_rmse"][0, 4])
    assert r["tile_max"] == pytest.approx(0.2 * np.sqrt(0.64))
    sse = 256 * (0.04 ** 2 + 0.08 ** 2 + 0.08 ** 2 + 0.2 ** 2 * 0.64)
    assert r["sse"] == pytest.approx(sse) and r["pixels"] == 4 * 256 and r["rmse"] == pytest.approx(np.sqrt(sse / 1024))
    # min_frames delays every freeze to the first checkpoint >= it
    r = replay(0, 64, 200, T, _const(seq), (1, 5))
    assert r["frames"].tolist() == [[64, 64, 64, 200, 64]]
    # everything frozen: the call ends at the freeze
    r = replay(0, 0, 4096, 1e9, _const(seq), (1, 5))
    assert r["frames"].tolist() == [[16] * 5] and r["frames_max"] == 16 and not r["active"].any()
    # a target below every tile: the uniform render of f0 + max_frames
    r = replay(8, 0, 40, 1e-12, lambda m, n: (np.full((1, 5), 0.01), np.full((1, 5), 256)), (1, 5))
    assert r["frames"].tolist() == [[48] * 5] and r["checkpoints"] == 2       # snapshot at 9, estimates at 18 and 36
    # no estimate within max_frames
    r = replay(0, 0, 3, 0.1, None, (1, 5))
    assert r["frames"].tolist() == [[3] * 5] and r["checkpoints"] == 0 and np.isnan(r["rmse"])


def test_tile_pixels_and_pixel_frames():
    assert tile_pixels(80, 96).tolist() == [[256] * 6] * 5
    assert tile_pixels(20, 37).tolist() == [[256, 256, 80], [64, 64, 20]]
    assert pixel_frames(np.array([[16, 32, 8], [8, 8, 8]]), 8, 20, 37) == 256 * 8 + 256 * 24


def test_struct_layout_matches_header():
    R = abi.AdaptiveResult
    assert C.sizeof(R) == 64
    names = ["frames_max", "frames_min", "tiles_x", "tiles_y", "tiles_active", "checkpoints", "pixel_frames", "pixels", "nonfinite", "sse",
             "rmse", "tile_max"]
    assert [f for f, _ in R._fields_] == names
    assert [getattr(R, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 60]
    body = re.search(r"typedef struct svr_adaptive_result \{(.*?)\} svr_adaptive_result;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(uint32_t|uint64_t|float|double)\s+([a-z_, ]+);", body)
    fields = [(t, n.strip()) for t, ns in decl for n in ns.split(",")]
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
    assert [n for _, n in fields] == names
    assert [ctype[t] for t, _ in fields] == [t for _, t in R._fields_]


def test_symbols():
    for name in ("svr_render_pathtracer_adaptive", "svr_get_adaptive_tiles"):
        assert name in abi.PROTOTYPES
        assert re.search(rf"\bint {name}\(", HEADER)
    so = abi.library_path()
    if so.exists() and shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True).stdout
        for name in ("svr_render_pathtracer_adaptive", "svr_get_adaptive_tiles"):
            assert re.search(rf"\bT {name}$", syms, flags=re.M), name


@pytest.fixture(scope="module")
def render_mhd(tmp_path_factory):
    exe = build_example(tmp_path_factory.mktemp("render_mhd"), strict=True)
    return exe


@pytest.mark.parametrize("value", ["0", "-1", "x"])
def test_render_mhd_rejects_bad_adaptive_target(render_mhd, tmp_path, value):
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), "-adaptive", value], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2, res.stdout + res.stderr
    assert "-adaptive needs a tile target RMSE > 0" in res.stderr


def test_render_mhd_accepts_adaptive_target(render_mhd, tmp_path):
    # parsed: the program goes on to the device / the volume (which does not exist) and fails there, not on its arguments
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), "-adaptive", "0.01", "-frames", "256"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode not in (0, 2), res.stdout + res.stderr
    assert "unknown argument" not in res.stderr and "-adaptive needs" not in res.stderr
    assert "-adaptive T" in subprocess.run([str(render_mhd)], capture_output=True, text=True, timeout=60).stderr
