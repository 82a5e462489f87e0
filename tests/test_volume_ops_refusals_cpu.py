"""The refusals of the volume-op entry points (svr_region_*, svr_volume_rank / _smooth): return code and the full text of
svr_last_error() for non-positive dimensions and for a connectivity / element that is not 6, 18 or 26, against the answers recorded in
tests/golden/volume_op_refusals.json (tests/golden/make_volume_op_refusals.py).  The checks stand before the device is touched, so the
library answers them without a GPU.  Every pointer is a real 64-byte buffer and every other argument is valid: a call whose check were
lost would go on with zero-sized or 4 x 4 x 4 work and fail the assertion."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi

GOLDEN = Path(__file__).resolve().parent / "golden" / "volume_op_refusals.json"
BAD_DIMS = [(0, 4, 4), (4, -1, 4), (4, 4, 0)]

# the calls: name -> {"args": the argument list, "answers": case -> [return value, error text]}; the argument notation is explained in
# tests/golden/make_volume_op_refusals.py, which holds the table
CALLS = json.loads(GOLDEN.read_text())


def cases(spec):
    """(case name, dims, the noun of the connectivity argument that is 7 or None) for an argument list"""
    out = [(f"dims {nx} x {ny} x {nz}", (nx, ny, nz), None) for nx, ny, nz in BAD_DIMS]
    nouns = [a[1] for a in spec if isinstance(a, list)] + (["connectivity"] if "params" in spec else [])
    return out + [(f"{noun} 7", (4, 4, 4), noun) for noun in nouns]


def refusal(lib, name, spec, dims, bad_noun):
    """calls `name` with the argument list `spec` and returns (return value, error text or None where the function does not report errors)"""
    restype, argtypes = abi.PROTOTYPES[name]
    keep, args = [], []
    for arg, ctype in zip(spec, argtypes):
        if arg in ("x", "y", "z"):
            args.append(dims["xyz".index(arg)])
        elif isinstance(arg, list):
            args.append(7 if arg[1] == bad_noun else 6)
        elif isinstance(arg, int):
            args.append(arg)
        else:
            buf = np.zeros(64, np.uint8)
            if arg == "ones":
                buf.view(np.uint32)[:] = 1
            elif arg == "spacing":
                buf.view(np.float64)[:] = 1.0
            elif arg == "params":
                params = abi.RegionParams.from_buffer(buf)
                assert lib.svr_region_params_default(C.byref(params)) == 0
                params.connectivity = 7 if bad_noun == "connectivity" else 6
            keep.append(buf)
            args.append(C.cast(buf.ctypes.data, ctype))
    lib.svr_clear_error()
    rc = getattr(lib, name)(*args)
    text = lib.svr_last_error().decode() if restype is C.c_int else None
    if restype is C.c_int:
        assert lib.svr_last_error_code() == rc
    lib.svr_clear_error()
    return int(rc), text


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    return lib


@pytest.mark.parametrize("name", list(CALLS))
def test_refusals_match_the_recording(lib, name):
    spec, answers = CALLS[name]["args"], CALLS[name]["answers"]
    assert [c for c, _, _ in cases(spec)] == list(answers), "the recording holds other cases: run tests/golden/make_volume_op_refusals.py"
    for case, dims, bad_noun in cases(spec):
        rc, text = refusal(lib, name, spec, dims, bad_noun)
        assert [rc, text] == answers[case], (name, case)
        if text is not None:
            assert rc == (-6 if bad_noun is None else -3) and name in text


def test_every_volume_op_with_dimensions_is_covered():
    header = (Path(__file__).resolve().parents[1] / "include" / "svr_abi.h").read_text()
    declared = re.findall(r"^\w+ (svr_\w+)\([^\n]*\bint nx, int ny, int nz\b", header, flags=re.M)
    assert declared[declared.index("svr_region_mask_words"):] == list(CALLS)
