#!/usr/bin/env python3
"""Record the fixtures of tests/test_refactor_pins_gpu.py from the HIP library as built: the local-majorant mode (pools and
straight line) and the env-NEE mode on small frames.  Needs an MI355X.  These pin this project's OWN arithmetic in the opt-in
modes (which have no oracle counterpart), so run it at the commit whose bits are to be kept, BEFORE the change that must keep them:

    python tests/golden/make_refactor_pins.py <commit hash of the tree that was built>"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from sunvolumerender_amd import _build, host  # noqa: E402
from tests import test_refactor_pins_gpu as pins  # noqa: E402


def main():
    commit = sys.argv[1]
    stamp = dict(commit=np.array(commit), kernel_source_hash=np.array(_build.kernel_source_hash()), compiler=np.array(pins.compiler_version()))
    dev = host.Device(0, fatal_errors=False)
    for name, depth, shift, sub in pins.LM_CASES:
        both = []
        for mode in (1, 2):
            got = pins.render_pin(dev, name, depth, shift, sub, lm=mode)
            assert all(v.dtype == np.float32 and v.max() > 0 for v in got.values())
            np.savez_compressed(pins.lm_file(name, depth, mode), **got, **stamp)
            both.append(got)
        same = all(np.array_equal(both[0][k].view(np.uint32), both[1][k].view(np.uint32)) for k in both[0])
        print(f"{name} depth {depth}: pools == straight line: {same}; {pins.lm_file(name, depth, 1).stat().st_size} bytes", flush=True)
    name, depth = pins.ENV_CASE
    got = pins.render_pin(dev, name, depth, env_nee=1, frames=(24,))
    default = pins.render_pin(dev, name, depth, frames=(24,))
    assert not np.array_equal(got["f24"], default["f24"]), "SVR_OPT_ENV_NEE rendered the default mode's bits: did it run?"
    np.savez_compressed(pins.env_file(name, depth), **got, **stamp)
    print(f"env NEE {name} depth {depth}: {pins.env_file(name, depth).stat().st_size} bytes; stamp {commit} {stamp['kernel_source_hash']} {stamp['compiler']}")


if __name__ == "__main__":
    main()
