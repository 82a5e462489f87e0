#!/usr/bin/env python3
"""Generates tests/golden/stb_ref_golden.npz: for every .hdr case of tests/test_io_cpu.py's stb comparison (and the sky map of
tests/test_io_gpu.py::test_env_map_file) the file and the floats the REFERENCE's stb_image.h (v2.12, utils/stb_image.h, built
where it lies into oracle/_ref/libstb_ref.so) decodes from it, plus the file the reference's stb_image_write.h (v1.02) writes for
the test's image.  With it those tests need no reference checkout; where oracle/_ref/libstb_ref.so is built they also check
the live library against this record.  Data only: inputs and expected outputs.
Run from the repo root where oracle/_ref/libstb_ref.so can be built:  python tests/golden/make_stb_ref_golden.py"""
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle import binding                                                  # noqa: E402
from tests.test_io_cpu import BAD_HDR_FILES, _hdr_cases, _stb_written_img    # noqa: E402
from tests.test_io_gpu import _sky_hdr                                      # noqa: E402


def main():
    assert binding.stb_ref() is not None, "needs the reference's stb headers (oracle/_ref/libstb_ref.so)"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        cases = _hdr_cases(d)
        binding.ref_write_hdr(d / "stbw.hdr", _stb_written_img())
        cases["stb_written"] = d / "stbw.hdr"
        cases["sky"] = _sky_hdr(d / "sky.hdr")
        for name, path in cases.items():
            rgb = binding.ref_loadf(path)
            assert rgb is not None and rgb.shape[2] == 3, name
            out[f"hdr_{name}_file"] = np.frombuffer(path.read_bytes(), dtype=np.uint8)
            out[f"hdr_{name}_rgb"] = rgb
        for name, data in BAD_HDR_FILES.items():
            (d / name).write_bytes(data)
            assert binding.ref_loadf(d / name) is None, name       # the tests expect stb to reject these
    np.savez_compressed(ROOT / "tests" / "golden" / "stb_ref_golden.npz", **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
