"""bench.py's launch contract, without a GPU: a WORLD_SIZE that disagrees with --gpus is an error (it used to run one GPU
and report n_gpus = 1 silently), and the multi-rank self-launch goes through torch.distributed.run."""
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_world_size_mismatch_is_an_error():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode != 0
    assert "WORLD_SIZE=3" in (res.stderr + res.stdout) and "--gpus 2" in (res.stderr + res.stdout)


def test_self_launch_builds_a_torchrun_command(monkeypatch):
    sys.path.insert(0, str(ROOT))
    import bench

    seen = {}
    monkeypatch.setattr(bench.subprocess, "call", lambda cmd, env=None: seen.update(cmd=cmd, env=env) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    assert bench.launch_ranks(4) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and cmd[-5].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_plain_run_leaves_the_extras_to_full(monkeypatch):
    """A plain run measures the headline only: the counting pass, the secondary workloads and the CPU baseline wait for --full."""
    sys.path.insert(0, str(ROOT))
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse_args()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 5, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "out"


def _frame(H, W):
    import numpy as np
    import torch

    rs = np.random.RandomState(0)
    hdr = rs.uniform(0, 9, H * W * 3).astype(np.float32)
    hdr[[4, 17, 31]] = np.nan, np.inf, -np.inf          # the accumulator keeps a non-finite sample for good
    hdr = torch.from_numpy(hdr)
    rgba = rs.randint(0, 256, (H, W, 4)).astype(np.uint8)
    return hdr, torch.from_numpy(rgba.view(np.int32).reshape(-1).copy()), rgba


def test_dump_outputs_writes_the_frame_as_float32(tmp_path):
    import numpy as np

    sys.path.insert(0, str(ROOT))
    import bench

    H, W = 6, 10
    hdr, img, rgba = _frame(H, W)
    bench.dump_outputs(tmp_path / "d", hdr, img, H, W)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["hdr.npy", "hdr_nonfinite.npy", "image.npy"]
    h, k, i = (np.load(tmp_path / "d" / f"{n}.npy") for n in ("hdr", "hdr_nonfinite", "image"))
    assert all(np.isfinite(a).all() for a in (h, k, i))
    want = hdr.numpy().reshape(H, W, 3)
    code = np.zeros(H * W * 3, dtype=np.float32)
    code[[4, 17, 31]] = 1, 2, 3
    assert k.dtype == np.float32 and np.array_equal(k.reshape(-1), code)
    assert h.dtype == np.float32 and h.shape == (H, W, 3) and np.array_equal(h[k == 0], want[k == 0]) and np.all(h[k != 0] == 0)
    assert i.dtype == np.float32 and i.shape == (H, W, 4) and np.array_equal(i, rgba.astype(np.float32))


def test_dump_outputs_keeps_a_fixed_row_sample_within_the_budget(tmp_path, monkeypatch):
    import numpy as np

    sys.path.insert(0, str(ROOT))
    import bench

    H, W = 50, 8
    hdr, img, rgba = _frame(H, W)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40 * W * 10)       # room for 10 of the 50 rows (12 + 12 + 16 bytes per pixel)
    bench.dump_outputs(tmp_path, hdr, img, H, W)
    rows = np.load(tmp_path / "rows.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, np.arange(0, H, 5))
    h, k, i = (np.load(tmp_path / f"{n}.npy") for n in ("hdr", "hdr_nonfinite", "image"))
    assert h.nbytes + k.nbytes + i.nbytes <= bench.DUMP_BUDGET_BYTES
    want = hdr.numpy().reshape(H, W, 3)[::5]
    assert np.array_equal(k != 0, ~np.isfinite(want)) and np.array_equal(h[k == 0], want[k == 0])
    assert np.array_equal(i, rgba[::5].astype(np.float32))
