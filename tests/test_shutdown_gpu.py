"""svr_shutdown with every lazily allocated buffer of the context in existence.  A child process (the C ABI keeps one context per
process) sets tiny_head up -- a volume, a transfer-function and an environment texture -- and then makes the library allocate what it
allocates on demand: a 2-frame render (scratch slots, record queues), a projection (the neighbour-max table of the volume texture), a
pick (the pixel list), a render under SVR_OPT_DENOISE_PREVIEW = 2 and SVR_OPT_NOISE_ESTIMATE = 1 (guides, filter scratch), an adaptive
call of 8 frames (tile list, snapshot, tile buffers), svr_pack_strips, and the destruction of one texture by hand.  The accumulator it
ends with is the 8 frames of the adaptive call, whose target no tile meets: it must equal the ordinary 8-frame render of this process
bit for bit.  Then svr_shutdown, and the child must leave with exit code 0 and no error recorded before the shutdown."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import scenes
from tests.util import assert_bit_exact, hip_frames

ROOT = Path(__file__).resolve().parents[1]

CHILD = """
import ctypes as C
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from sunvolumerender_amd import abi, host, scenes

dev = host.Device(0, fatal_errors=False)
lib = dev.lib
sc = scenes.make_scene("tiny_head")
cv = host.Canvas(dev, sc.width, sc.height)
scenes.apply_to_canvas(sc, cv)                                 # volume, transfer-function and environment textures
W, H = sc.width, sc.height
cv.paint_frames(2, sync=True)
cv.paint_projection(abi.PROJ_MIP, sync=True)
hits = cv.pick([(W // 2, H // 2), (0, 0)])
assert len(hits) == 2
cv.SetDenoisePreview(2)
cv.SetNoiseEstimate(True)
cv.ReStartRender()
cv.paint_frames(2, sync=True)
cv.ReStartRender()
res = cv.paint_adaptive(1e-9, max_frames=8, sync=True)
assert (res.frames_min, res.frames_max) == (8, 8), (res.frames_min, res.frames_max)
rows = int(lib.svr_strip_rows_owned(H, 8, 1, 2))
packed = dev.malloc(rows * W * 3 * 4)
dev.check(lib.svr_pack_strips(C.c_void_p(packed), cv.renderParams.hdrBuffer, W, H, 8, 1, 2))
dev.synchronize()
vox = np.zeros((9, 10, 11), np.uint16)
extra = lib.svr_create_volume_texture(vox.ctypes.data_as(C.c_void_p), 11, 10, 9, 0, abi.LAYOUT_AUTO)
dev.check()
dev.check(lib.svr_destroy_texture(extra))
np.save(%(out)r, cv.read_hdr())
code = lib.svr_last_error_code()
print("error code before the shutdown:", code, lib.svr_last_error().decode())
lib.svr_shutdown()                                             # (the canvas is NOT closed: its textures and buffers are the library's to free)
print("shutdown returned")
sys.exit(0 if code == 0 else 3)
"""


@pytest.mark.gpu
def test_shutdown_with_everything_allocated(hip_dev, tmp_path):
    out = tmp_path / "hdr.npy"
    res = subprocess.run([sys.executable, "-c", CHILD % {"root": str(ROOT), "out": str(out)}], capture_output=True, text=True, timeout=300,
                         cwd=str(ROOT))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "error code before the shutdown: 0" in res.stdout and "shutdown returned" in res.stdout, res.stdout + res.stderr
    sc = scenes.make_scene("tiny_head")
    hdr, _, _ = hip_frames(hip_dev, sc, 8, batch=True, count=False)
    assert_bit_exact(np.load(out), hdr, "accumulator of the child before its shutdown vs the ordinary 8-frame render")
