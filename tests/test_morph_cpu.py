"""The mask calls without a GPU: the test-side reference (tests/morph_ref.py) against scipy.ndimage and the algebra of the contract
(duality, open <= M <= close, idempotence), the ABI of the new symbols and constants, every refusal (arguments are checked before the
device is touched), the arguments of examples/render_mhd.cpp, and the conditions the fixtures of tests/test_morph_gpu.py have to meet,
asserted on the reference."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, scenes
from tests import morph_ref as mr
from tests import region_ref as rr
from tests.test_region_cpu import BONE, BRAIN, bone_seed
from tests.cpp_example import build_example

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
STRUCTURES = {6: 1, 18: 2, 26: 3}


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    lib.svr_clear_error()
    return lib


def head_regions():
    """(brain, bone) of tiny_head as the region reference grows them."""
    vox = scenes.make_scene("tiny_head").vox
    brain, _ = rr.reference("head", vox, [BRAIN[2]], BRAIN[0], BRAIN[1], 6)
    bone, _ = rr.reference("head", vox, [bone_seed(vox)], BONE[0], BONE[1], 6)
    return brain, bone


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("element", mr.ELEMENTS)
def test_reference_against_scipy(element):
    ndi = pytest.importorskip("scipy.ndimage")
    st = ndi.generate_binary_structure(3, STRUCTURES[element])
    for shape, density, seed in (((9, 10, 37), 0.5, 1), ((7, 12, 33), 0.1, 2), ((12, 9, 20), 0.9, 3), ((1, 1, 40), 0.5, 4), ((5, 1, 3), 0.6, 5)):
        m = mr.random_mask(shape, density, seed)
        for radius in (1, 2, 3):
            d = ndi.binary_dilation(m, st, iterations=radius, border_value=0)
            e = ndi.binary_erosion(m, st, iterations=radius, border_value=1)
            assert np.array_equal(mr.dilate(m, element, radius), d) and np.array_equal(mr.erode(m, element, radius), e)
            o, c = mr.morph(m, mr.OPEN, element, radius), mr.morph(m, mr.CLOSE, element, radius)
            assert np.array_equal(o, ndi.binary_dilation(e, st, iterations=radius, border_value=0))
            assert np.array_equal(c, ndi.binary_erosion(d, st, iterations=radius, border_value=1))
            # duality, open <= M <= close, idempotence
            assert np.array_equal(mr.erode(m, element, radius), ~mr.dilate(~m, element, radius))
            assert not (o & ~m).any() and not (m & ~c).any()
            assert np.array_equal(mr.morph(o, mr.OPEN, element, radius), o) and np.array_equal(mr.morph(c, mr.CLOSE, element, radius), c)
        marker = mr.random_mask(shape, 0.03, seed + 10)
        assert np.array_equal(mr.reconstruct(marker, m, element), ndi.binary_propagation(marker & m, structure=st, mask=m))
        assert np.array_equal(mr.fill_holes(m, element), ndi.binary_fill_holes(m, structure=st))
    # a hole proper, and the default of scipy is background connectivity 6
    box = np.zeros((9, 9, 9), dtype=bool)
    box[2:7, 2:7, 2:7] = True
    box[4, 4, 4] = False
    assert np.array_equal(mr.fill_holes(box, 6), ndi.binary_fill_holes(box)) and mr.fill_holes(box, 6).sum() == 125


def test_reference_detach_by_hand():
    m = mr.two_balls()
    assert m.shape == mr.TWO_BALL_SHAPE
    out, status = mr.detach(m, [mr.TWO_BALL_SEED], 6, 1)
    core = mr.erode(m, 6, 1)
    # the opening's component around the seed, cut back to the mask; the bridge (one voxel wide) is not in it
    assert status == rr.OK and not (out & ~m).any() and not out[9, 9, 30:44].any() and (core & out).sum() > 0
    assert np.array_equal(out, mr.dilate(mr.reconstruct(mr.dilate(mr.points(m.shape, [mr.TWO_BALL_SEED]), 6, 1), core, 6), 6, 1) & m)


def test_combine_reference():
    a, b = mr.random_mask((3, 4, 40), 0.5, 1), mr.random_mask((3, 4, 40), 0.5, 2)
    assert np.array_equal(mr.combine(a, b, mr.ANDNOT), a & ~b) and np.array_equal(mr.combine(a, None, mr.NOT), ~a)
    assert np.array_equal(mr.combine(a, b, mr.XOR), mr.combine(mr.combine(a, b, mr.OR), mr.combine(a, b, mr.AND), mr.ANDNOT))


# ---------------------------------------------------------------- ABI
def test_symbols_and_constants(lib):
    names = ["svr_region_morph", "svr_region_combine", "svr_region_reconstruct", "svr_region_fill_holes", "svr_region_detach",
             "svr_region_mask_last_ms"]
    raw = C.CDLL(str(abi.library_path()))
    for n in names:
        assert n in abi.PROTOTYPES and hasattr(raw, n), n
        assert re.search(rf"\b{n}\s*\(", HEADER), n

    def define(name):
        m = re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", HEADER)
        assert m, name
        return int(m.group(1))

    assert (abi.MORPH_DILATE, abi.MORPH_ERODE, abi.MORPH_OPEN, abi.MORPH_CLOSE) == tuple(define("SVR_MORPH_" + n) for n in ("DILATE", "ERODE", "OPEN", "CLOSE")) \
        == (mr.DILATE, mr.ERODE, mr.OPEN, mr.CLOSE)
    assert (abi.MASK_AND, abi.MASK_OR, abi.MASK_ANDNOT, abi.MASK_XOR, abi.MASK_NOT) == tuple(define("SVR_MASK_" + n) for n in ("AND", "OR", "ANDNOT", "XOR", "NOT")) \
        == (mr.AND, mr.OR, mr.ANDNOT, mr.XOR, mr.NOT)
    assert len({abi.MORPH_DILATE, abi.MORPH_ERODE, abi.MORPH_OPEN, abi.MORPH_CLOSE}) == 4
    assert abi.MORPH_MAX_RADIUS == define("SVR_MORPH_MAX_RADIUS") == mr.MAX_RADIUS == 32
    ms = C.c_float(7.0)
    assert lib.svr_region_mask_last_ms(C.byref(ms)) == 0 and ms.value >= 0.0              # (0 when no mask call has run in this process)
    assert lib.svr_region_mask_last_ms(None) == -4
    lib.svr_clear_error()


# ---------------------------------------------------------------- refusals: all are decided before the device is touched
A, B, OUT = 0x10000, 0x20000, 0x30000                   # three "device pointers" 64 KiB apart: masks of 4 x 4 x 4 (64 bytes) do not overlap


def _refused(lib, name, rc, code, word):
    msg = lib.svr_last_error().decode()
    last = lib.svr_last_error_code()
    lib.svr_clear_error()
    assert rc == last == code and name in msg and word in msg, (name, rc, last, msg)


def _morph(lib, inp=A, dims=(4, 4, 4), op=abi.MORPH_DILATE, element=6, radius=1, out=OUT):
    return lib.svr_region_morph(C.c_void_p(inp), *dims, op, element, radius, C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [
    (dict(inp=None), -4, "null"), (dict(out=None), -4, "null"),
    (dict(dims=(0, 4, 4)), -6, "dimensions"), (dict(dims=(4, -1, 4)), -6, "dimensions"), (dict(dims=(4, 4, 0)), -6, "dimensions"),
    (dict(dims=(2048, 1024, 1025)), -6, "2^31"),
    (dict(op=0), -3, "op"), (dict(op=5), -3, "op"), (dict(element=4), -3, "element"), (dict(element=27), -3, "element"),
    (dict(radius=0), -3, "radius"), (dict(radius=33), -3, "radius"),
    (dict(out=A), -3, "overlap"), (dict(out=A + 60), -3, "overlap"), (dict(inp=A + 32, out=A), -3, "overlap"),
])
def test_morph_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_morph", _morph(lib, **kw), code, word)


def _combine(lib, a=A, b=B, dims=(4, 4, 4), op=abi.MASK_AND, out=OUT):
    return lib.svr_region_combine(C.c_void_p(a), C.c_void_p(b), *dims, op, C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [
    (dict(a=None), -4, "null"), (dict(out=None), -4, "null"), (dict(b=None), -4, "null"), (dict(b=None, op=abi.MASK_XOR), -4, "null"),
    (dict(dims=(4, 0, 4)), -6, "dimensions"), (dict(dims=(2**16, 2**16, 1)), -6, "2^31"),
    (dict(op=0), -3, "op"), (dict(op=6), -3, "op"), (dict(op=abi.MASK_NOT), -3, "NULL"),
])
def test_combine_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_combine", _combine(lib, **kw), code, word)


def _reconstruct(lib, marker=A, cand=B, dims=(4, 4, 4), conn=6, max_sweeps=0, out=OUT, sweeps=True):
    n = C.c_uint32(77)
    rc = lib.svr_region_reconstruct(C.c_void_p(marker), C.c_void_p(cand), *dims, conn, max_sweeps, C.c_void_p(out), C.byref(n) if sweeps else None)
    assert n.value == 77                                                                # nothing is written on a refusal
    return rc


@pytest.mark.parametrize("kw, code, word", [
    (dict(marker=None), -4, "null"), (dict(cand=None), -4, "null"), (dict(out=None), -4, "null"), (dict(out=None, sweeps=False), -4, "null"),
    (dict(dims=(4, 4, -4)), -6, "dimensions"), (dict(dims=(2**31 - 1, 2, 1)), -6, "2^31"),
    (dict(conn=0), -3, "connectivity"), (dict(conn=8), -3, "connectivity"),
    (dict(out=A), -3, "overlap"), (dict(out=B), -3, "overlap"), (dict(out=B + 4), -3, "overlap"),
])
def test_reconstruct_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_reconstruct", _reconstruct(lib, **kw), code, word)


def _fill(lib, inp=A, dims=(4, 4, 4), conn=6, max_sweeps=0, out=OUT):
    return lib.svr_region_fill_holes(C.c_void_p(inp), *dims, conn, max_sweeps, C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [
    (dict(inp=None), -4, "null"), (dict(out=None), -4, "null"), (dict(dims=(0, 0, 0)), -6, "dimensions"), (dict(dims=(2048, 1024, 1025)), -6, "2^31"),
    (dict(conn=4), -3, "connectivity"), (dict(conn=19), -3, "connectivity"), (dict(out=A), -3, "overlap"), (dict(out=A - 4), -3, "overlap"),
])
def test_fill_holes_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_fill_holes", _fill(lib, **kw), code, word)


def _detach(lib, inp=A, dims=(4, 4, 4), seeds=((0, 0, 0),), nseeds=None, element=6, radius=1, conn=6, max_sweeps=0, out=OUT, status=True):
    xyz = (C.c_int32 * (3 * max(len(seeds or ()), 1)))(*[c for s in seeds or () for c in s])
    st = C.c_int32(55)
    rc = lib.svr_region_detach(C.c_void_p(inp), *dims, xyz if seeds is not None else None, len(seeds or ()) if nseeds is None else nseeds,
                               element, radius, conn, max_sweeps, C.c_void_p(out), C.byref(st) if status else None)
    assert st.value == 55
    return rc


@pytest.mark.parametrize("kw, code, word", [
    (dict(inp=None), -4, "null"), (dict(out=None), -4, "null"), (dict(status=False), -4, "null"), (dict(seeds=None, nseeds=1), -4, "null"),
    (dict(dims=(4, 0, 4)), -6, "dimensions"), (dict(dims=(2048, 1024, 1025)), -6, "2^31"),
    (dict(nseeds=0), -3, "nseeds"), (dict(seeds=((0, 0, 0),) * 65), -3, "nseeds"),
    (dict(seeds=((4, 0, 0),)), -3, "seed"), (dict(seeds=((0, -1, 0),)), -3, "seed"), (dict(seeds=((1, 1, 1), (0, 0, 4))), -3, "seed"),
    (dict(element=8), -3, "element"), (dict(radius=0), -3, "radius"), (dict(radius=33), -3, "radius"),
    (dict(conn=7), -3, "connectivity"), (dict(out=A), -3, "overlap"),
])
def test_detach_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_detach", _detach(lib, **kw), code, word)


# ---------------------------------------------------------------- conditions on the fixtures of the GPU tests
def test_head_fixtures_have_the_stated_sizes():
    brain, bone = head_regions()
    assert brain.sum() == 13709 and bone.sum() == 5410
    assert mr.fill_holes(brain, 6).sum() == 13943
    out, status = mr.detach(brain, [(24, 24, 25)], 6, 1)
    assert (out.sum(), status) == (13663, rr.OK)
    out, status = mr.detach(brain, [(24, 23, 26)], 26, 2)
    assert (out.sum(), status) == (13457, rr.OK)
    out, status = mr.detach(brain, [(24, 24, 24)], 6, 1)                                # the seed lies outside the opening
    assert (out.sum(), status) == (0, rr.EMPTY) and brain[24, 24, 24]
    assert mr.fill_holes(bone, 6).sum() == 21844
    assert mr.fill_holes(bone, 26).sum() == 5410                                        # the shell leaks through corners
    assert mr.morph(bone, mr.CLOSE, 26, 1).sum() == 5432


def test_two_ball_fixture():
    m = mr.two_balls()
    assert m.shape == (20, 20, 72) and m.sum() == 1848
    filled = mr.fill_holes(m, 6)
    assert (filled & ~m).sum() == 19 and filled[9, 9, 20] and not m[9, 9, 20]
    assert mr.second_ball(m) > 800
    for (element, radius), want in (((6, 1), 882), ((6, 2), 818), ((26, 1), 900), ((18, 2), None)):
        out, status = mr.detach(m, [mr.TWO_BALL_SEED], element, radius, 6)
        if want is None:
            assert status == rr.EMPTY and not out.any()
        else:
            assert status == rr.OK and out.sum() == want and mr.second_ball(out) == 0
    # the serpentine as a mask: one component under 6
    s, seed = mr.serpentine_mask()
    assert np.array_equal(mr.reconstruct(mr.points(s.shape, [seed]), s, 6), s)


# ---------------------------------------------------------------- examples/render_mhd.cpp: the clean-up arguments
@pytest.fixture(scope="module")
def render_mhd(tmp_path_factory):
    exe = build_example(tmp_path_factory.mktemp("render_mhd_morph"), strict=True)
    return exe


GROW = ["-grow", "1", "2", "0", "10"]


@pytest.mark.parametrize("args", [GROW + ["-detach", "0"], GROW + ["-detach", "33"], GROW + ["-detach"], GROW + ["-open", "0"], GROW + ["-open", "x"],
                                  GROW + ["-close", "-1"], GROW + ["-dilate", "40"], GROW + ["-erode"], GROW + ["-open", "1", "-element", "8"],
                                  ["-detach", "1"], ["-fillholes"]])
def test_render_mhd_rejects_bad_cleanup_arguments(render_mhd, tmp_path, args):
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), *args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.strip(), (res.returncode, res.stderr)


def test_render_mhd_usage_names_the_cleanup_steps(render_mhd):
    err = subprocess.run([str(render_mhd)], capture_output=True, text=True, timeout=60).stderr
    for word in ("-detach R", "-fillholes", "-open R", "-close R", "-dilate R", "-erode R", "-element 6|18|26"):
        assert word in err, word
