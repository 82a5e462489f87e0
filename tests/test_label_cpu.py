"""The component calls without a GPU: the test-side reference (tests/label_ref.py) against scipy.ndimage -- as arrays, not up to a
permutation --, the ABI of the new symbols, constants and struct, every refusal (arguments are checked before the device is touched), the
new arguments of examples/render_mhd.cpp, and the conditions the fixtures of tests/test_label_gpu.py have to meet, asserted on the
reference."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import label_ref as lr
from tests import region_ref as rr
from tests.test_region_cpu import BONE, BRAIN, THIN
from tests.cpp_example import build_example

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
LABEL_SOURCE = (ROOT / "sunvolumerender_amd" / "csrc" / "svr_label.hip").read_text()
STRUCTURES = {6: 1, 18: 2, 26: 3}
WINDOWS = {"brain": BRAIN[:2], "bone": BONE[:2], "thin": THIN[:2]}
HEAD_COUNTS = {"brain": {6: 675, 18: 296, 26: 164}, "bone": {6: 1, 18: 1, 26: 1}, "thin": {6: 562, 18: 8, 26: 6}}
NOISE_SHAPE = (17, 16, 256)
NOISE_COUNTS = {(0, 250): {6: 5653, 18: 277, 26: 78}, (0, 649): {6: 164, 18: 1, 26: 1}}


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    lib.svr_clear_error()
    return lib


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("conn", lr.CONNS)
def test_reference_against_scipy(conn):
    ndi = pytest.importorskip("scipy.ndimage")
    st = ndi.generate_binary_structure(3, STRUCTURES[conn])
    for shape in (rr.EDGE_SHAPES[0], rr.EDGE_SHAPES[5], rr.EDGE_SHAPES[9], (1, 1, 64), (12, 9, 20)):
        vox = rr.noise_volume(shape, seed=11)
        for k, density in enumerate(lr.DENSITIES):
            m = lr.random_mask(shape, density, 20 + k)
            labels, count = lr.label(m, conn)
            want, n = ndi.label(m, structure=st)
            assert count == n and np.array_equal(labels, want.astype(np.uint32)), (shape, density)
            if count == 0:
                continue
            t = lr.table(labels, count, vox)
            idx = np.arange(1, count + 1)
            assert np.array_equal(t["voxels"], ndi.sum(m, want, idx).astype(np.uint32))
            assert np.array_equal(t["sum"], ndi.sum(vox.astype(np.float64), want, idx).astype(np.uint64))
            lin = np.arange(m.size).reshape(shape)
            firsts = [int(lin[p]) for p in ndi.minimum_position(lin, want, idx)]
            assert t["first"].tolist() == firsts and firsts == sorted(firsts)
            for i, sl in enumerate(ndi.find_objects(want)):
                assert t["bbox_min"][i].tolist() == [sl[2].start, sl[1].start, sl[0].start]
                assert t["bbox_max"][i].tolist() == [sl[2].stop - 1, sl[1].stop - 1, sl[0].stop - 1]
            assert np.array_equal(lr.table(labels, count)["sum"], np.zeros(count, dtype=np.uint64))


def test_reference_selection_by_hand():
    sizes = [5, 20, 1, 20, 32, 20]
    assert lr.kept_labels(sizes, 0, 0) == [1, 2, 3, 4, 5, 6] and lr.kept_labels(sizes, 20, 0) == [2, 4, 5, 6]
    assert lr.kept_labels(sizes, 0, 1) == [5] and lr.kept_labels(sizes, 0, 2) == [2, 5] and lr.kept_labels(sizes, 0, 3) == [2, 4, 5]   # ties: the lower label
    assert lr.kept_labels(sizes, 21, 3) == [5] and lr.kept_labels(sizes, 33, 0) == []
    labels = np.array([[[1, 0, 2, 2, 0, 3]]], dtype=np.uint32)
    assert lr.select(labels, [1, 0, 1, 0]).tolist() == [[[False, False, True, True, False, False]]]      # entry 0 is ignored
    mask, kept = lr.select_by_size(labels, 3, 2, 0)
    assert kept == 1 and mask.tolist() == [[[False, False, True, True, False, False]]]


# ---------------------------------------------------------------- ABI
def test_symbols_constants_and_struct(lib):
    names = ["svr_region_threshold", "svr_region_label", "svr_region_label_table", "svr_region_select", "svr_region_select_by_size",
             "svr_region_label_last_ms"]
    raw = C.CDLL(str(abi.library_path()))
    for n in names:
        assert n in abi.PROTOTYPES and hasattr(raw, n), n
        assert re.search(rf"\b{n}\s*\(", HEADER), n
    m = re.search(r"#define\s+SVR_REGION_ERR_LABEL\s+\((-?\d+)\)", HEADER)
    assert m and int(m.group(1)) == abi.REGION_ERR_LABEL == -10 and abi.REGION_ERR_LABEL != abi.REGION_ERR_SWEEPS
    assert re.search(r"typedef struct svr_region_component \{\s*/\* 40 bytes \*/", HEADER)
    K = abi.RegionComponent
    assert C.sizeof(K) == 40 == host.COMPONENT_DTYPE.itemsize
    assert [getattr(K, f).offset for f in lr.COMPONENT_FIELDS] == [0, 4, 8, 20, 32] == [host.COMPONENT_DTYPE.fields[f][1] for f in lr.COMPONENT_FIELDS]
    m = re.search(r"#define\s+SVR_LABEL_SCAN_BLOCK\s+(\d+)", LABEL_SOURCE)
    assert m and int(m.group(1)) == abi.LABEL_SCAN_BLOCK == host.LABEL_SCAN_BLOCK
    ms = C.c_float(7.0)
    assert lib.svr_region_label_last_ms(C.byref(ms)) == 0 and ms.value >= 0.0
    assert lib.svr_region_label_last_ms(None) == -4
    lib.svr_clear_error()


# ---------------------------------------------------------------- refusals: all are decided before the device is touched
A, B, OUT = 0x10000, 0x20000, 0x30000                   # "device pointers": nothing is read or written through them


def _refused(lib, name, rc, code, word):
    msg = lib.svr_last_error().decode()
    last = lib.svr_last_error_code()
    lib.svr_clear_error()
    assert rc == last == code and name in msg and word in msg, (name, rc, last, msg)


def _box(b):
    return None if b is None else (C.c_int32 * 3)(*b)


def _threshold(lib, vox=A, dims=(4, 4, 4), lo=0, hi=10, box_min=None, box_max=None, out=OUT):
    return lib.svr_region_threshold(C.c_void_p(vox), *dims, 1, lo, hi, _box(box_min), _box(box_max), C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [
    (dict(vox=None), -4, "null"), (dict(out=None), -4, "null"),
    (dict(dims=(0, 4, 4)), -6, "dimensions"), (dict(dims=(4, -1, 4)), -6, "dimensions"), (dict(dims=(4, 4, 0)), -6, "dimensions"),
    (dict(dims=(2048, 1024, 1025)), -6, "2^31"),
    (dict(lo=11), -3, "window"), (dict(hi=65536), -3, "window"),
    (dict(box_min=(0, 0, 0)), -3, "box"), (dict(box_max=(3, 3, 3)), -3, "box"),
    (dict(box_min=(2, 0, 0), box_max=(1, 3, 3)), -3, "box"), (dict(box_min=(0, 4, 0), box_max=(3, 9, 3)), -3, "box"),
    (dict(box_min=(0, 0, -5), box_max=(3, 3, -1)), -3, "box"),
])
def test_threshold_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_threshold", _threshold(lib, **kw), code, word)


def _label(lib, inp=A, dims=(4, 4, 4), conn=6, labels=OUT, count=True):
    k = C.c_uint32(77)
    rc = lib.svr_region_label(C.c_void_p(inp), *dims, conn, C.c_void_p(labels), C.byref(k) if count else None)
    assert k.value == 77                                                                # nothing is written on a refusal
    return rc


@pytest.mark.parametrize("kw, code, word", [
    (dict(inp=None), -4, "null"), (dict(labels=None), -4, "null"), (dict(count=False), -4, "null"),
    (dict(dims=(4, 0, 4)), -6, "dimensions"), (dict(dims=(2**16, 2**16, 1)), -6, "2^31"),
    (dict(conn=0), -3, "connectivity"), (dict(conn=8), -3, "connectivity"), (dict(conn=27), -3, "connectivity"),
])
def test_label_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_label", _label(lib, **kw), code, word)


def _table(lib, labels=A, vox=None, dims=(4, 4, 4), count=1, table=OUT):
    return lib.svr_region_label_table(C.c_void_p(labels), C.c_void_p(vox), *dims, 1, count, C.c_void_p(table))


@pytest.mark.parametrize("kw, code, word", [
    (dict(labels=None), -4, "null"), (dict(table=None), -4, "null"), (dict(dims=(4, 4, -4)), -6, "dimensions"),
    (dict(dims=(2**31 - 1, 2, 1)), -6, "2^31"), (dict(count=0), -3, "count"), (dict(count=0, vox=B), -3, "count"),
])
def test_table_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_label_table", _table(lib, **kw), code, word)


def _select(lib, labels=A, dims=(4, 4, 4), count=1, keep=B, out=OUT):
    return lib.svr_region_select(C.c_void_p(labels), *dims, count, C.c_void_p(keep), C.c_void_p(out))


@pytest.mark.parametrize("kw, code, word", [
    (dict(labels=None), -4, "null"), (dict(keep=None), -4, "null"), (dict(out=None), -4, "null"),
    (dict(dims=(0, 0, 0)), -6, "dimensions"), (dict(dims=(2048, 1024, 1025)), -6, "2^31"), (dict(count=0), -3, "count"),
])
def test_select_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_select", _select(lib, **kw), code, word)


def _by_size(lib, labels=A, dims=(4, 4, 4), count=1, table=B, min_voxels=0, largest_k=0, out=OUT, kept=True):
    k = C.c_uint32(77)
    rc = lib.svr_region_select_by_size(C.c_void_p(labels), *dims, count, C.c_void_p(table), min_voxels, largest_k, C.c_void_p(out),
                                       C.byref(k) if kept else None)
    assert k.value == 77
    return rc


@pytest.mark.parametrize("kw, code, word", [
    (dict(labels=None), -4, "null"), (dict(table=None), -4, "null"), (dict(out=None), -4, "null"), (dict(kept=False), -4, "null"),
    (dict(dims=(4, 0, 4)), -6, "dimensions"), (dict(dims=(2048, 1024, 1025)), -6, "2^31"), (dict(count=0), -3, "count"),
])
def test_select_by_size_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_select_by_size", _by_size(lib, **kw), code, word)


# ---------------------------------------------------------------- conditions on the fixtures of the GPU tests
def head_mask(name):
    lo, hi = WINDOWS[name]
    return lr.threshold(scenes.make_scene("tiny_head").vox, lo, hi)


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_head_fixtures_have_the_stated_components(name):
    m = head_mask(name)
    for conn in lr.CONNS:
        labels, count = lr.labelled("head-" + name, m, conn)
        assert count == HEAD_COUNTS[name][conn], (name, conn, count)
        assert np.array_equal(labels != 0, m)
    if name == "brain":
        assert m.sum() == BRAIN[4] == 14709
        sizes18 = sorted(np.bincount(lr.labelled("head-brain", m, 18)[0].reshape(-1))[1:].tolist(), reverse=True)
        assert sizes18[:4] == [13709, 32, 20, 20]                                       # largest_k = 3 falls on the tie
        sizes6 = np.bincount(lr.labelled("head-brain", m, 6)[0].reshape(-1))[1:]
        assert sizes6.max() == 13709 and (sizes6 >= 10).sum() == 5


def test_noise_and_serpentine_fixtures():
    vox = rr.noise_volume(NOISE_SHAPE)
    for (lo, hi), counts in NOISE_COUNTS.items():
        for conn in lr.CONNS:
            assert lr.labelled(f"noise-{hi}", lr.threshold(vox, lo, hi), conn)[1] == counts[conn], (hi, conn)
    s = rr.serpentine()[0] > 0
    labels, count = lr.labelled("serpentine", s, 6)
    assert count == 1 and s.sum() == 4427 and (labels == 1).sum() == 4427
    c = lr.checkerboard()
    assert c.shape == (64, 64, 64) and c.sum() == 131072
    m = lr.last_largest()
    for conn in lr.CONNS:
        labels, count = lr.label(m, conn)
        sizes = np.bincount(labels.reshape(-1))[1:]
        assert count == 3 and sizes.argmax() == 2                                       # the largest component starts last


def test_gpu_shapes_cross_the_blocks_of_the_scan():
    """One block of a level of svr_region_label's renumbering scan covers LABEL_SCAN_BLOCK words (SVR_LABEL_SCAN_BLOCK in
    csrc/svr_label.hip): the GPU shapes must hold more than one block, and -- the scan having further levels -- more than one block of
    blocks."""
    block = host.LABEL_SCAN_BLOCK
    shapes = rr.EDGE_SHAPES + [lr.CHECKER_SHAPE, lr.SCAN3_SHAPE]
    words = {s: host.region_mask_words(s) for s in shapes}
    assert any(block < w <= block * block for w in words.values()) and host.region_label_scan_levels(lr.CHECKER_SHAPE) == 2
    assert words[lr.SCAN3_SHAPE] > block * block and host.region_label_scan_levels(lr.SCAN3_SHAPE) == 3
    assert words[lr.SCAN3_SHAPE] < block * block + 2 * block                            # as small as the constant allows
    assert all(np.prod(s) < 300000 for s in shapes)
    assert host.region_label_scan_levels((1, 1, 1)) == 1 and host.region_label_scan_levels((1, 256, 32)) == 1
    # the largest volume of the contract (2^31 voxels in rows of one voxel is not it: 2^26 words of 32) needs a fourth level
    assert host.region_label_scan_levels((1024, 1024, 2048)) == 4


# ---------------------------------------------------------------- examples/render_mhd.cpp: the component arguments
@pytest.fixture(scope="module")
def render_mhd(tmp_path_factory):
    exe = build_example(tmp_path_factory.mktemp("render_mhd_label"), strict=True)
    return exe


GROW = ["-grow", "1", "2", "0", "10"]
THRESHOLD = ["-threshold", "0", "10"]


@pytest.mark.parametrize("args", [["-threshold", "10"], ["-threshold", "10", "5"], ["-threshold", "0", "65536"], ["-threshold", "x", "5"],
                                  GROW + THRESHOLD, THRESHOLD + ["-largest", "0"], THRESHOLD + ["-largest"], THRESHOLD + ["-largest", "x"],
                                  THRESHOLD + ["-minsize", "0"], THRESHOLD + ["-minsize", "-3"], GROW + ["-minsize"],
                                  ["-largest", "1"], ["-minsize", "5"]])
def test_render_mhd_rejects_bad_component_arguments(render_mhd, tmp_path, args):
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), *args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.strip(), (res.returncode, res.stderr)


def test_render_mhd_usage_names_the_component_steps(render_mhd):
    err = subprocess.run([str(render_mhd)], capture_output=True, text=True, timeout=60).stderr
    for word in ("-threshold LO HI", "-largest K", "-minsize N"):
        assert word in err, word
