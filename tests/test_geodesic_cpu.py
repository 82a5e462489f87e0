"""The geodesic calls without a GPU: the test-side reference (tests/geodesic_ref.py: a Jacobi iteration on packed keys) against an independent
heap Dijkstra on every small fixture, svr_region_geodesic_weights against its definition, the ABI of the new symbols and constants, every
refusal (arguments are checked before the device is touched), the two-ball phantom by hand, the -split argument of
examples/render_mhd.cpp, and the conditions the fixtures of tests/test_geodesic_gpu.py have to meet, asserted on the reference."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import distance_ref as dr
from tests import geodesic_ref as gr
from tests import label_ref as lr
from tests.cpp_example import build_example

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "svr_abi.h").read_text()
SOURCE = (ROOT / "sunvolumerender_amd" / "csrc" / "svr_geo_relax.hpp").read_text()        # the tile constants


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    lib.svr_clear_error()
    return lib


def same_pair(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("density", gr.DENSITIES)
def test_reference_against_dijkstra_random(density):
    domain, labels = gr.random_case(density)
    for name, w in gr.WEIGHT_SETS.items():
        same_pair(gr.cached_geodesic(f"random {density}", labels, domain, w), gr.dijkstra(labels, domain, w), (density, name))


def test_reference_against_dijkstra_small_fixtures():
    for shape in gr.FLAT_SHAPES:
        domain = gr.random_domain(shape, 0.8, 3)
        labels = gr.random_markers(shape, 3, 4)
        for name, w in gr.WEIGHT_SETS.items():
            same_pair(gr.geodesic(labels, domain, w), gr.dijkstra(labels, domain, w), (shape, name))
    for axis, middle in gr.TIE_CASES:
        for swapped in (False, True):
            labels, domain, _ = gr.tie_line(axis, middle, swapped)
            same_pair(gr.geodesic(labels, domain), gr.dijkstra(labels, domain), (axis, middle, swapped))
    labels, domain = gr.serpentine()
    same_pair(gr.cached_geodesic("serpentine", labels, domain), gr.dijkstra(labels, domain), "serpentine")
    m = gr.two_ball_phantom()
    cores, _ = lr.label(dr.ball(m, dr.ERODE, gr.PHANTOM_R2), 26)
    for w in (gr.CHAMFER, gr.PHANTOM_6_WEIGHTS, (1, 0, 0, 0, 0, 0, 0), (2, 2, 2, 3, 3, 3, 0)):
        same_pair(gr.geodesic(cores, m, w), gr.dijkstra(cores, m, w), w)


def test_reference_by_hand():
    domain = np.ones((1, 3, 5), dtype=bool)
    domain[0, 1, 1:4] = False
    labels = np.zeros((1, 3, 5), dtype=np.uint32)
    labels[0, 0, 0], labels[0, 1, 2] = 5, 8                                               # (the second lies outside the domain)
    dist, zones = gr.geodesic(labels, domain)
    assert dist[0].tolist() == [[0, 3, 6, 9, 12], [3, gr.NONE, gr.NONE, gr.NONE, 13], [6, 7, 10, 13, 16]]
    assert zones[0].tolist() == [[5, 5, 5, 5, 5], [5, 0, 0, 0, 5], [5, 5, 5, 5, 5]]
    dist6, _ = gr.geodesic(labels, domain, gr.WEIGHT_SETS["6-only"])
    assert dist6[0, 2].tolist() == [6, 9, 12, 15, 18]
    only_x, zx = gr.geodesic(labels, domain, (1, 0, 0, 0, 0, 0, 0))
    assert only_x[0, 0].tolist() == [0, 1, 2, 3, 4] and (only_x[0, 1:] == gr.NONE).all() and not zx[0, 1:].any()
    assert gr.seed_labels([(1, 0, 0), (2, 0, 0), (1, 0, 0)], (1, 1, 4))[0, 0].tolist() == [0, 1, 2, 0]
    z = np.array([[[4, 4, 2, 2, 0, 9]]], dtype=np.uint32)
    assert gr.zone_cut(z, 6)[0, 0].tolist() == [True, False, True, True, False, True]


# ---------------------------------------------------------------- svr_region_geodesic_weights
def _weights(lib, spacing, connectivity, shape, w=True, unit=True, sp=True):
    nz, ny, nx = shape
    s = (C.c_double * 3)(*spacing)
    out, u = (C.c_uint32 * 7)(*([77] * 7)), C.c_double(-1.0)
    rc = lib.svr_region_geodesic_weights(s if sp else None, connectivity, nx, ny, nz, out if w else None, C.byref(u) if unit else None)
    return rc, tuple(out), u.value


@pytest.mark.parametrize("spacing, connectivity, shape, k", [
    ((1.0, 1.0, 1.0), 26, (64, 64, 64), 3), ((1.0, 1.0, 1.0), 18, (64, 64, 64), 3), ((1.0, 1.0, 1.0), 6, (64, 64, 64), 3),
    ((0.9, 0.9, 1.5), 26, (48, 48, 48), 3), ((0.9, 0.9, 1.5), 18, (300, 512, 512), 3),
    ((1.0, 1.0, 1.0), 26, (1024, 1024, 1024), 1),                                         # 14 and 7 do not fit 2^30 voxels, 3 does
    ((1.0, 1.0, 1.0), 6, (2, 1024, 2 ** 20), 1),                                            # 2 (2^31 - 1) is the limit itself
    ((1.0, 1.0, 1.0), 26, (1, 2, 2 ** 30), 0), ((3.0, 2.0, 1.0), 26, (1, 1, 1), 3),
])
def test_geodesic_weights_follow_their_definition(lib, spacing, connectivity, shape, k):
    want_w, want_unit, want_k = gr.weights_from_spacing(spacing, connectivity, shape)
    assert want_k == k and gr.fits(want_w, shape)
    if k < 3:                                                                             # the next finer unit must not fit
        assert not gr.fits(gr.weights_at(spacing, connectivity, k + 1)[0], shape)
    rc, w, unit = _weights(lib, spacing, connectivity, shape)
    assert rc == 0 and w == want_w and unit == want_unit == min(spacing) / 2 ** k
    assert host.geodesic_weights(spacing, connectivity, shape, lib) == (want_w, want_unit)
    assert all((w[c] == 0) == (c >= gr.CLASSES[connectivity]) for c in range(7))
    if spacing == (1.0, 1.0, 1.0) and k == 3:
        assert w[:gr.CLASSES[connectivity]] == (8, 8, 8, 11, 11, 11, 14)[:gr.CLASSES[connectivity]]
    if spacing == (0.9, 0.9, 1.5) and connectivity == 26:
        # unit 0.1125: 0.9 -> 8, 1.5 -> 13.33, sqrt(1.62) -> 11.31, sqrt(3.06) -> 15.55, sqrt(3.87) -> 17.49
        assert w == (8, 8, 13, 11, 16, 16, 17)


def test_geodesic_weights_refusals(lib):
    with pytest.raises(ValueError):
        gr.weights_from_spacing((1.0, 1.0, 3.0), 6, (2, 1024, 2 ** 20))                   # the z move costs at least 3: 3 (2^31 - 1) is too much
    _refused(lib, "svr_region_geodesic_weights", _weights(lib, (1.0, 1.0, 3.0), 6, (2, 1024, 2 ** 20))[0], -3, "32 bits")
    _refused(lib, "svr_region_geodesic_weights", _weights(lib, (1.0, 1.0, 1e7), 6, (8, 8, 8))[0], -3, "32 bits")
    for spacing in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        with pytest.raises(ValueError):
            gr.weights_from_spacing(spacing, 26, (4, 4, 4))
        rc, w, unit = _weights(lib, spacing, 26, (4, 4, 4))
        assert w == (77,) * 7 and unit == -1.0                                            # nothing is written on a refusal
        _refused(lib, "svr_region_geodesic_weights", rc, -3, "spacing")
    for conn in (0, 7, 27, -6):
        _refused(lib, "svr_region_geodesic_weights", _weights(lib, (1.0, 1.0, 1.0), conn, (4, 4, 4))[0], -3, "connectivity")
    for kw in (dict(sp=False), dict(w=False), dict(unit=False)):
        _refused(lib, "svr_region_geodesic_weights", _weights(lib, (1.0, 1.0, 1.0), 26, (4, 4, 4), **kw)[0], -4, "null")
    _refused(lib, "svr_region_geodesic_weights", _weights(lib, (1.0, 1.0, 1.0), 26, (4, 0, 4))[0], -6, "dimensions")
    _refused(lib, "svr_region_geodesic_weights", _weights(lib, (1.0, 1.0, 1.0), 26, (2048, 1024, 1025))[0], -6, "2^31")
    with pytest.raises(host.SvrError):
        host.geodesic_weights((1.0, 1.0, 1e7), 6, (8, 8, 8), lib)


# ---------------------------------------------------------------- ABI
NAMES = ["svr_region_geodesic", "svr_region_seed_labels", "svr_region_geodesic_weights", "svr_region_split", "svr_region_zone_cut",
         "svr_region_geodesic_last_ms", "svr_region_geodesic_default_max_sweeps"]


def test_symbols_and_constants(lib):
    raw = C.CDLL(str(abi.library_path()))
    for n in NAMES:
        assert n in abi.PROTOTYPES and hasattr(raw, n), n
        assert re.search(rf"\b{n}\s*\(", HEADER), n
    m = re.search(r"#define\s+SVR_GEO_NONE\s+(\w+)", HEADER)
    assert m and int(m.group(1).rstrip("u"), 0) == abi.GEO_NONE == gr.NONE == 0xFFFFFFFF
    assert abi.GEO_TILE == gr.TILE
    m = re.search(r"constexpr int GX = (\d+), GY = (\d+), GZ = (\d+);", SOURCE)
    assert m and tuple(int(t) for t in m.groups()) == gr.TILE
    assert "svr_geodesic.hip" in (ROOT / "sunvolumerender_amd" / "_build.py").read_text()
    for dev_method in ("region_geodesic", "region_seed_labels", "region_split", "region_zone_cut", "region_geodesic_last_ms"):
        assert callable(getattr(host.Device, dev_method))
    ms = C.c_float(7.0)
    assert lib.svr_region_geodesic_last_ms(C.byref(ms)) == 0 and ms.value >= 0.0
    assert lib.svr_region_geodesic_last_ms(None) == -4
    lib.svr_clear_error()


def test_default_sweep_cap(lib):
    """min(64 + 16 T, 65536) over tiles of 32 x 8 x 8 voxels; 0 for no volume."""
    for dims, tiles in (((72, 21, 19), 27), ((32, 8, 8), 1), ((33, 9, 9), 8), ((70, 40, 9), 30), ((512, 512, 512), 65536)):
        assert lib.svr_region_geodesic_default_max_sweeps(*dims) == min(64 + 16 * tiles, 65536), dims
    assert lib.svr_region_geodesic_default_max_sweeps(0, 4, 4) == 0


# ---------------------------------------------------------------- refusals: all are decided before the device is touched
A, B, OUT, OUT2 = 0x100000, 0x200000, 0x300000, 0x400000     # "device pointers": nothing is read or written through them


def _refused(lib, name, rc, code, word):
    msg = lib.svr_last_error().decode()
    last = lib.svr_last_error_code()
    lib.svr_clear_error()
    assert rc == last == code and name in msg and word in msg, (name, rc, last, msg)


def _p(v):
    return None if v is None else C.c_void_p(v)


def _w7(weights):
    return None if weights is None else (C.c_uint32 * 7)(*weights)


def _w3(weights):
    return None if weights is None else (C.c_uint32 * 3)(*weights)


DIMS = [(dict(dims=(0, 4, 4)), -6, "dimensions"), (dict(dims=(4, -1, 4)), -6, "dimensions"), (dict(dims=(4, 4, 0)), -6, "dimensions"),
        (dict(dims=(2048, 1024, 1025)), -6, "2^31"), (dict(dims=(2 ** 16, 2 ** 16, 1)), -6, "2^31")]
# the overflow bound wmax (voxels - 1) <= 0xFFFFFFFE at the last admissible and the first refused weight: 64 voxels leave 63 moves,
# 0xFFFFFFFE // 63 = 68174084; two voxels leave one move of any weight but 0xFFFFFFFF; 2^31 voxels only the weight 1 (2 (2^31 - 1) = LIMIT)
STEPS = [(dict(steps=(0,) * 7), -3, "0"), (dict(steps=(1, 1, 1, 1, 1, 1, 68174085)), -3, "overflow"),
         (dict(steps=(68174085, 0, 0, 0, 0, 0, 0)), -3, "overflow"), (dict(steps=(0xFFFFFFFF, 1, 1, 0, 0, 0, 0), dims=(2, 1, 1)), -3, "overflow"),
         (dict(steps=(1, 1, 3, 0, 0, 0, 0), dims=(2048, 1024, 1024)), -3, "overflow"), (dict(steps=None, dims=(1024, 1024, 1024)), -3, "overflow")]
ADMITTED = [dict(steps=(1, 1, 1, 1, 1, 1, 68174084)), dict(steps=(0xFFFFFFFE, 0, 0, 0, 0, 0, 0), dims=(2, 1, 1)),
            dict(steps=(1, 2, 2, 0, 0, 0, 0), dims=(2048, 1024, 1024)), dict(steps=(0xFFFFFFFF,) * 7, dims=(1, 1, 1)),
            dict(steps=None, dims=(512, 512, 512))]


def test_the_overflow_bound_is_the_contracts():
    for kw in ADMITTED:
        nx, ny, nz = kw.get("dims", (4, 4, 4))
        assert gr.fits(kw["steps"] or gr.CHAMFER, (nz, ny, nx)), kw
    for kw, code, word in STEPS:
        if word == "overflow":
            nx, ny, nz = kw.get("dims", (4, 4, 4))
            assert not gr.fits(kw["steps"] or gr.CHAMFER, (nz, ny, nx)), kw
    assert 68174084 * 63 <= gr.LIMIT < 68174085 * 63 and 2 * (2 ** 31 - 1) == gr.LIMIT and 5 * (512 ** 3 - 1) <= gr.LIMIT < 5 * (1024 ** 3 - 1)


def _geodesic(lib, labels=A, domain=B, dims=(4, 4, 4), steps=gr.CHAMFER, max_sweeps=0, dist=OUT, zones=OUT2):
    sweeps = C.c_uint32(77)
    rc = lib.svr_region_geodesic(_p(labels), _p(domain), *dims, _w7(steps), max_sweeps, _p(dist), _p(zones), C.byref(sweeps))
    assert sweeps.value == 77                                                             # nothing is written on a refusal
    return rc


@pytest.mark.parametrize("kw, code, word", [
    (dict(labels=None), -4, "null"), (dict(domain=None), -4, "null"), (dict(dist=None, zones=None), -4, "null"),
    (dict(dist=A), -3, "overlap"), (dict(dist=A + 252), -3, "overlap"), (dict(dist=B), -3, "overlap"), (dict(zones=B + 60), -3, "overlap"),
    (dict(zones=A + 4), -3, "overlap"), (dict(dist=OUT, zones=OUT + 128), -3, "overlap"), (dict(dist=A, zones=A), -3, "overlap")] + DIMS + STEPS)
def test_geodesic_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_geodesic", _geodesic(lib, **kw), code, word)


def _seed_labels(lib, seeds=((1, 2, 3),), n=None, dims=(4, 4, 4), out=OUT, null_seeds=False):
    xyz = (C.c_int32 * (3 * max(len(seeds), 1)))(*[c for s in seeds for c in s])
    return lib.svr_region_seed_labels(None if null_seeds else xyz, len(seeds) if n is None else n, *dims, _p(out))


@pytest.mark.parametrize("kw, code, word", [
    (dict(null_seeds=True), -4, "null"), (dict(out=None), -4, "null"), (dict(n=0), -3, "nseeds"), (dict(seeds=((0, 0, 0),) * 65), -3, "nseeds"),
    (dict(seeds=((4, 0, 0),)), -3, "outside"), (dict(seeds=((0, 0, 0), (0, -1, 0))), -3, "outside"), (dict(seeds=((0, 0, 4),)), -3, "outside")] + DIMS)
def test_seed_labels_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_seed_labels", _seed_labels(lib, **kw), code, word)


def _split(lib, inp=A, dims=(4, 4, 4), dist_weights=None, r2=1, connectivity=26, steps=None, zones=OUT, outs=(True, True, True)):
    count, lost, sweeps = C.c_uint32(77), C.c_uint32(77), C.c_uint32(77)
    refs = [C.byref(v) if on else None for v, on in zip((count, lost, sweeps), outs)]
    rc = lib.svr_region_split(_p(inp), *dims, _w3(dist_weights), r2, connectivity, _w7(steps), 0, _p(zones), *refs)
    assert (count.value, lost.value, sweeps.value) == (77, 77, 77)                        # nothing is written on a refusal
    return rc


@pytest.mark.parametrize("kw, code, word", [
    (dict(inp=None), -4, "null"), (dict(zones=None), -4, "null"), (dict(outs=(False, True, True)), -4, "null"), (dict(outs=(True, False, True)), -4, "null"),
    (dict(connectivity=0), -3, "connectivity"), (dict(connectivity=8), -3, "connectivity"), (dict(zones=A), -3, "overlap"), (dict(inp=OUT + 252), -3, "overlap"),
    (dict(dist_weights=(0, 1, 1)), -3, "weight"), (dict(dist_weights=(1, 1, 0)), -3, "weight"),
    (dict(dist_weights=(2, 1, 1), dims=(65536, 1, 1)), -3, "overflow"), (dict(dist_weights=(1, 0xFFFFFFFF, 0xFFFFFFFF)), -3, "overflow")] + DIMS + STEPS[:4])
def test_split_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_split", _split(lib, **kw), code, word)


def _zone_cut(lib, zones=A, dims=(4, 4, 4), connectivity=26, out=OUT):
    return lib.svr_region_zone_cut(_p(zones), *dims, connectivity, _p(out))


@pytest.mark.parametrize("kw, code, word", [(dict(zones=None), -4, "null"), (dict(out=None), -4, "null"), (dict(connectivity=4), -3, "connectivity"),
                                            (dict(connectivity=27), -3, "connectivity"), (dict(out=A), -3, "overlap"), (dict(out=A + 252), -3, "overlap"),
                                            (dict(zones=OUT + 12), -3, "overlap")] + DIMS)
def test_zone_cut_refusals(lib, kw, code, word):
    _refused(lib, "svr_region_zone_cut", _zone_cut(lib, **kw), code, word)


# ---------------------------------------------------------------- conditions on the fixtures of the GPU tests
def test_gpu_shapes_span_three_tiles_per_axis():
    for shape in (gr.GPU_SHAPE,):
        for n, t in zip(shape[::-1], gr.TILE):
            assert -(-n // t) >= 3 and n % t != 0, (shape, n, t)
    nz, ny, nx = gr.SERPENTINE_SHAPE
    assert -(-nx // gr.TILE[0]) >= 3 and -(-ny // gr.TILE[1]) >= 3
    assert any(s[2] == 33 for s in gr.FLAT_SHAPES) and any(s[2] > 2 * gr.TILE[0] for s in gr.FLAT_SHAPES)
    assert any(s[1] > 2 * gr.TILE[1] for s in gr.FLAT_SHAPES) and any(s[0] > 2 * gr.TILE[2] for s in gr.FLAT_SHAPES) and (1, 1, 1) in gr.FLAT_SHAPES


def _flip(labels):
    """The labels in reverse order (l -> 2^32 - l keeps them non-zero and distinct)."""
    return np.where(labels != 0, (2 ** 32 - labels.astype(np.int64)) % 2 ** 32, 0).astype(np.uint32)


@pytest.mark.parametrize("density", gr.DENSITIES)
def test_gpu_cases_have_ties_pockets_and_markers_outside(density):
    domain, labels = gr.random_case(density)
    assert (labels != 0).sum() == 40 and ((labels != 0) & ~domain).any() and ((labels != 0) & domain).sum() >= 10
    assert int(labels.max()) > 2 ** 31 and len(np.unique(labels)) == 41
    for name, w in gr.WEIGHT_SETS.items():
        dist, zones = gr.cached_geodesic(f"random {density}", labels, domain, w)
        reached = dist != gr.NONE
        # pockets that no marker reaches: wherever the moves leave the domain in pieces (26-moves join a domain of density 0.7 up)
        assert (domain & ~reached).any() == (density < 0.5 or name == "6-only"), (density, name, "pockets")
        assert not (reached & ~domain).any() and ((zones != 0) == reached).all()
        # a voxel whose zone changes when the order of the labels is reversed is reached by two markers at the same distance
        dflip, zflip = gr.geodesic(_flip(labels), domain, w)
        assert np.array_equal(dflip, dist)
        assert (_flip(zflip) != zones).any(), (density, name, "no tie")


def test_tie_lines_by_hand():
    for axis, middle in gr.TIE_CASES:
        for swapped in (False, True):
            labels, domain, mid = gr.tie_line(axis, middle, swapped)
            dist, zones = gr.geodesic(labels, domain)
            assert domain.sum() == 11 and dist[mid] == 15 and zones[mid] == 3
            assert sorted(np.bincount(zones[domain])[[3, 7]].tolist()) == [5, 6]
            assert mid[2 - axis] == middle and middle in (gr.TILE[axis] - 1, gr.TILE[axis])


def test_serpentine_by_hand():
    labels, domain = gr.serpentine()
    dist, zones = gr.cached_geodesic("serpentine", labels, domain)
    assert (labels != 0).sum() == 1 and int(dist[domain].max()) == gr.SERPENTINE_MAX and (zones[domain] == 9).all()
    # the Euclidean way would be short: the corridor is what makes it long
    assert gr.SERPENTINE_MAX > 3 * 10 * gr.SERPENTINE_SHAPE[2]


# ---------------------------------------------------------------- the split phantom
def test_phantom_by_hand():
    m = gr.two_ball_phantom()
    assert m.shape == gr.PHANTOM_SHAPE == (24, 24, 40) and lr.label(m, 26)[1] == 1 and lr.label(m, 6)[1] == 1
    d2 = dr.distance_map(m, (1, 1, 1), dr.TO_UNSET)
    assert lr.label(d2 > 36, 26)[1] == 2 and lr.label(d2 > 25, 26)[1] == 1
    assert np.array_equal(d2 > 36, dr.ball(m, dr.ERODE, 36))
    zones, count, lost = gr.cached(("phantom", 26), lambda: gr.split(m, gr.PHANTOM_R2, 26))
    assert count == 2 and lost == 0 and tuple(np.bincount(zones.reshape(-1))[1:].tolist()) == gr.PHANTOM_ZONES["chamfer"] == (3019, 2917)
    zones6, count6, lost6 = gr.split(m, gr.PHANTOM_R2, 26, step_weights=gr.PHANTOM_6_WEIGHTS)
    assert count6 == 2 and lost6 == 0 and tuple(np.bincount(zones6.reshape(-1))[1:].tolist()) == gr.PHANTOM_ZONES["6"] == (3024, 2912)
    assert sum(gr.PHANTOM_ZONES["chamfer"]) == sum(gr.PHANTOM_ZONES["6"]) == m.sum()
    cut = gr.zone_cut(zones, 26)
    assert lr.label(cut, 26)[1] == 2 and not (cut & ~m).any() and (zones[m & ~cut] == 2).all()
    for k in (1, 2):
        assert lr.label(zones == k, 26)[1] == 1                                           # an influence zone is connected
    none, count0, lost0 = gr.split(m, gr.PHANTOM_R2_NONE, 26)                             # no voxel is that deep
    assert int(d2.max()) == 82 < gr.PHANTOM_R2_NONE
    assert count0 == 0 and not none.any() and lost0 == m.sum()


def test_thin_pieces_fixture():
    m = gr.thin_pieces_mask()
    zones, count, lost = gr.cached(("thin",), lambda: gr.split(m, gr.THIN_R2, 18, dist_weights=gr.THIN_DIST_WEIGHTS))
    assert count == 12 and lost == 861 and lr.label(m, 18)[1] == 25 and m.sum() == 8470
    assert lost == (m & (zones == 0)).sum() and len(np.unique(zones)) == count + 1


# ---------------------------------------------------------------- examples/render_mhd.cpp: the -split argument
@pytest.fixture(scope="module")
def render_mhd(tmp_path_factory):
    exe = build_example(tmp_path_factory.mktemp("render_mhd_geodesic"), strict=True)
    return exe


THRESHOLD = ["-threshold", "0", "10"]


@pytest.mark.parametrize("args", [THRESHOLD + ["-split"], THRESHOLD + ["-split", "0"], THRESHOLD + ["-split", "-2"], THRESHOLD + ["-split", "x"],
                                  THRESHOLD + ["-split", "1.5mm"], THRESHOLD + ["-split", "inf"], THRESHOLD + ["-split", "nan"], ["-split", "2"]])
def test_render_mhd_rejects_bad_split_arguments(render_mhd, tmp_path, args):
    res = subprocess.run([str(render_mhd), str(tmp_path / "missing.mhd"), *args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 2 and res.stderr.strip(), (res.returncode, res.stderr)


def test_render_mhd_usage_names_the_split_step(render_mhd):
    err = subprocess.run([str(render_mhd)], capture_output=True, text=True, timeout=60).stderr
    assert "-split L" in err
