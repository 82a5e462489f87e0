"""What the tests of the C++ examples share: the g++ line that builds examples/*.cpp against include/ and libsvr_hip.so, and the
float32 re-derivation of the eye distance that include/sunvolumerender/canvas.hpp computes."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi

ROOT = Path(__file__).resolve().parents[1]


def build_example(tmp_path, name="render_mhd", strict=False, link=True):
    """Builds examples/<name>.cpp into tmp_path / <name> with plain g++ (strict: -Wall -Werror; link: with an rpath to the library's
    directory, so the program runs as it is) and returns the program's path.  Skips where there is no g++."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = Path(tmp_path) / name
    libdir = abi.library_path().parent
    cmd = ["g++", "-std=c++14", "-O1", *(["-Wall", "-Werror"] if strict else []), f"-I{ROOT / 'include'}", str(ROOT / "examples" / f"{name}.cpp"),
           "-o", str(exe), f"-L{libdir}", "-lsvr_hip", *([f"-Wl,-rpath,{libdir}"] if link else [])]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def cpp_canvas_eye(canvas):
    """The eye distance of the C++ Canvas for the volume the Python `canvas` has loaded.  Its ZoomToExtent (canvas.hpp, from
    gui/canvas.cpp:191-197) evaluates the tangent and the division in double and rounds once; the Python Canvas works in float32
    throughout, so the two may differ by an ulp -- which a grazing pixel of a picture can show -- and must agree to 1e-5."""
    f32 = np.float32
    span = f32(f32(max(canvas.volumeSize)) * f32(1.5))
    eye = float(f32(float(span) / (2 * math.tan(float(f32(f32(canvas.fov) * f32(0.5)) * f32(0.01745329251994329576923690768489))))))
    assert abs(eye - canvas.eyeDist) <= 1e-5 * eye
    return eye
