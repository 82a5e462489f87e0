"""The reference of the grow-from-seeds calls (tests/growcut_ref.py) against itself -- Jacobi against a heap Dijkstra, gain 0 against the
geodesic reference, the saturated solution under random relaxation orders -- and what the library answers without a GPU:
svr_region_growcut_params_default and every refusal of the section, return code and error text.  The refusals stand before the device is
touched; every pointer is a real host buffer, and a call whose check were lost would go on to initialise a device."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi
from tests import geodesic_ref as gr
from tests import growcut_ref as gc

SMALL = (5, 6, 9)                                        # for the sequential methods


# ------------------------------------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("shape", [gc.TILED_SHAPES[0], gc.ONE_TILE] + gr.FLAT_SHAPES, ids=str)
def test_jacobi_equals_dijkstra(shape):
    combos = gc.combinations(shape)
    if int(np.prod(shape)) > 500:                                                         # the heap is slow: a covering part of the product
        combos = gc.covering_combinations()
    for kind, density, name, gs in combos:
        vox, labels, domain = gc.case(shape, kind, density)
        want = gc.cached_case(shape, kind, density, name, gs)
        got = gc.dijkstra(vox, labels, domain, gc.WEIGHT_SETS[name], *gs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (shape, kind, density, name, gs)


def test_the_cases_have_ties_pockets_and_contrast():
    """What the GPU tests rely on: small values give equal-cost paths (a changed tie rule would change zones), sparse domains leave
    unreached pockets, and the image term changes the zones."""
    shape = gc.TILED_SHAPES[0]
    vox, labels, domain = gc.case(shape, "small", 0.45)
    cost, zones = gc.cached_case(shape, "small", 0.45, "26", (1, 0))
    assert (domain & (cost == gc.NONE)).any() and (zones[~domain] == 0).all() and (cost[~domain] == gc.NONE).all()
    flat = gc.cached_case(shape, "small", 0.45, "26", (0, 0))
    assert not np.array_equal(flat[1], zones)
    # ties: giving the LARGER label to equal keys changes the result
    big = np.where(labels != 0, 4 - labels, 0).astype(np.uint32)                         # classes 1 .. 3 reversed
    mirrored = gc.growcut(vox, big, domain, gc.WEIGHT_SETS["26"], 1, 0)
    back = np.where(mirrored[1] != 0, 4 - mirrored[1], 0)
    assert np.array_equal(mirrored[0], cost) and not np.array_equal(back, zones)


@pytest.mark.parametrize("name", list(gc.WEIGHT_SETS))
def test_gain_zero_is_the_geodesic_reference(name):
    shape = gc.TILED_SHAPES[0]
    for density in gr.DENSITIES:
        vox, labels, domain = gc.case(shape, "full", density)
        want = gr.geodesic(labels, domain, gc.WEIGHT_SETS[name])
        for shift in (0, 3):
            got = gc.growcut(vox, labels, domain, gc.WEIGHT_SETS[name], 0, shift)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_saturated_line():
    for swapped in (False, True):
        vox, labels = gc.saturating_line(swapped)
        cost, zones = gc.growcut(vox, labels, None, gc.default_weights(6), gc.SAT_GAIN, 0)
        move = 1 + gc.SAT_GAIN * 65535
        assert move <= gc.MAX_MOVE and 2 * move < gc.CAP < 3 * move
        n = gc.SAT_SHAPE[2]
        assert cost[0, 0, :3].tolist() == [0, move, 2 * move] and cost[0, 0, -3:].tolist() == [2 * move, move, 0]
        assert (cost[0, 0, 3:n - 3] == gc.CAP).all() and int((cost == gc.CAP).sum()) == n - 6
        assert (zones[0, 0, 3:n - 3] == 3).all()                                          # the plateau carries the smaller label
        near7 = zones[0, 0, :3] if not swapped else zones[0, 0, -3:]
        assert (near7 == 7).all()
        d = gc.dijkstra(vox, labels, None, gc.default_weights(6), gc.SAT_GAIN, 0)
        assert np.array_equal(d[0], cost) and np.array_equal(d[1], zones)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_saturated_solution_does_not_depend_on_the_order(seed):
    """Sequential Gauss-Seidel over a shuffled voxel list: on the saturating line, and on a small volume whose costs saturate."""
    rng = np.random.default_rng(seed)
    vox, labels = gc.saturating_line()
    order = [tuple(p) for p in rng.permutation(np.argwhere(np.ones(gc.SAT_SHAPE, dtype=bool))).tolist()]
    want = gc.growcut(vox, labels, None, gc.default_weights(6), gc.SAT_GAIN, 0)
    got = gc.gauss_seidel(vox, labels, None, gc.default_weights(6), gc.SAT_GAIN, 0, order)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    vox = (np.indices(SMALL).sum(axis=0) % 2 * 65535).astype(np.uint16)                  # a checkerboard: every 6-move crosses full contrast
    labels = gc.class_markers(SMALL, 4, 8)
    domain = gr.random_domain(SMALL, 0.8, 9)
    want = gc.growcut(vox, labels, domain, gc.default_weights(6), 30000, 0)
    assert (want[0] == gc.CAP).any() and (want[0] < gc.CAP).any()
    order = [tuple(p) for p in rng.permutation(np.argwhere(np.ones(SMALL, dtype=bool))).tolist()]
    got = gc.gauss_seidel(vox, labels, domain, gc.default_weights(6), 30000, 0, order)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_seed_classes_and_label_paint_reference():
    shape = (3, 4, 5)
    out = gc.seed_classes([(0, 0, 0), (4, 3, 2), (0, 0, 0)], [5, 6, 7], shape)
    assert out[0, 0, 0] == 5 and out[2, 3, 4] == 6 and np.count_nonzero(out) == 2
    mask = np.zeros(shape, dtype=bool)
    mask[0, 0, :2] = True
    assert gc.label_paint(out, mask, 9, False)[0, 0, :2].tolist() == [9, 9]
    assert gc.label_paint(out, mask, 9, True)[0, 0, :2].tolist() == [5, 9]


# ------------------------------------------------------------------------------------------------ the library without a GPU
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    return lib


def answer(lib, rc):
    text = lib.svr_last_error().decode()
    assert lib.svr_last_error_code() == rc
    lib.svr_clear_error()
    return int(rc), text


def test_params_default(lib):
    for conn, classes in ((6, 3), (18, 6), (26, 7)):
        p = abi.GrowcutParams()
        p.contrast_shift, p.max_sweeps = 9, 9
        assert lib.svr_region_growcut_params_default(C.byref(p), conn) == 0
        assert list(p.step_weights) == [1] * classes + [0] * (7 - classes) == list(gc.default_weights(conn))
        assert (p.contrast_gain, p.contrast_shift, p.max_sweeps) == (1, 0, 0)
    assert C.sizeof(abi.GrowcutParams) == 40 and C.sizeof(abi.GrowcutInfo) == 24
    rc, text = answer(lib, lib.svr_region_growcut_params_default(None, 6))
    assert rc == -4 and "svr_region_growcut_params_default" in text
    p = abi.GrowcutParams()
    rc, text = answer(lib, lib.svr_region_growcut_params_default(C.byref(p), 7))
    assert rc == -3 and "svr_region_growcut_params_default" in text and "6, 18 or 26" in text


class Args:
    """Valid arguments of svr_region_growcut on a 4 x 4 x 4 volume in one host buffer, which the refusals never read or write."""

    def __init__(self, lib):
        self.lib = lib
        self.buf = np.full(4096, 0x5A, np.uint8)
        base = self.buf.ctypes.data
        self.vox, self.markers, self.domain, self.cost, self.zones = base, base + 512, base + 1024, base + 2048, base + 3072
        self.dims = (C.c_int32 * 3)(4, 4, 4)
        self.params = abi.GrowcutParams()
        assert lib.svr_region_growcut_params_default(C.byref(self.params), 26) == 0
        self.info = abi.GrowcutInfo()
        self.info.sweeps = 77

    def call(self, **over):
        a = dict(vox=self.vox, dims=self.dims, on_dev=1, markers=self.markers, domain=self.domain, params=C.byref(self.params), cost=self.cost,
                 zones=self.zones, info=C.byref(self.info))
        a.update(over)
        ptr = lambda v: v if v is None or not isinstance(v, int) else C.c_void_p(v)     # noqa: E731
        rc = self.lib.svr_region_growcut(ptr(a["vox"]), a["dims"], a["on_dev"], ptr(a["markers"]), ptr(a["domain"]), a["params"], ptr(a["cost"]),
                                         ptr(a["zones"]), a["info"])
        rc, text = answer(self.lib, rc)
        assert "svr_region_growcut" in text
        assert (self.buf == 0x5A).all() and self.info.sweeps == 77                        # nothing written
        return rc, text


def test_growcut_null_and_dimension_refusals(lib):
    a = Args(lib)
    for name in ("vox", "dims", "markers", "params"):
        rc, text = a.call(**{name: None})
        assert rc == -4 and "null argument" in text, name
    rc, text = a.call(cost=None, zones=None)
    assert rc == -4 and "both outputs are null" in text
    for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        rc, text = a.call(dims=(C.c_int32 * 3)(*bad))
        assert rc == -6 and "bad dimensions" in text, bad
    rc, text = a.call(dims=(C.c_int32 * 3)(2048, 2048, 513))
    assert rc == -6 and "more than 2^31 voxels" in text


def test_growcut_parameter_refusals(lib):
    a = Args(lib)

    def with_params(weights=None, gain=1, shift=0):
        p = abi.GrowcutParams()
        assert lib.svr_region_growcut_params_default(C.byref(p), 26) == 0
        if weights is not None:
            p.step_weights[:] = weights
        p.contrast_gain, p.contrast_shift = gain, shift
        return a.call(params=C.byref(p))
    rc, text = with_params(weights=[0] * 7)
    assert rc == -3 and "all seven step weights are 0" in text
    rc, text = with_params(gain=65536)
    assert rc == -3 and "contrast_gain" in text and "65536" in text
    rc, text = with_params(shift=16)
    assert rc == -3 and "contrast_shift" in text and "16" in text
    # wmax + gain * (65535 >> shift) > 0x7FFFFFFF
    for weights, gain, shift in (([1] * 7, 65535, 0), ([1] * 7, 32769, 0), ([0x7FFFFFFF, 0, 0, 0, 0, 0, 0], 1, 15), ([0x80000000, 1, 1, 0, 0, 0, 0], 0, 0),
                                 ([0x7FFFFFFF - 32767 * 65535 + 1] + [1] * 6, 32767, 0)):
        assert gc.refused(weights, gain, shift)
        rc, text = with_params(weights, gain, shift)
        assert rc == -3 and "0x7FFFFFFF" in text, (weights, gain, shift)
    assert not gc.refused([0x7FFFFFFF - 32767 * 65535] + [1] * 6, 32767, 0) and not gc.refused([1] * 7, gc.SAT_GAIN - 1, 0)


def test_growcut_overlap_refusals(lib):
    a = Args(lib)
    for over in (dict(cost=a.markers + 4), dict(zones=a.markers + 4), dict(cost=a.markers), dict(zones=a.domain), dict(cost=a.domain - 252),
                 dict(cost=a.vox + 124), dict(zones=a.vox)):
        rc, text = a.call(**over)
        assert rc == -3 and "must not overlap an input" in text, over
    rc, text = a.call(zones=a.cost + 252)
    assert rc == -3 and "the two outputs must not overlap" in text


def test_seed_classes_refusals(lib):
    buf = np.full(1024, 0x5A, np.uint8)
    out = C.c_void_p(buf.ctypes.data)
    dims = (C.c_int32 * 3)(4, 5, 6)

    def call(seeds, classes, n=None, dims=dims, out=out):
        xyz = None if seeds is None else (C.c_int32 * (3 * len(seeds)))(*[c for s in seeds for c in s])
        cls = None if classes is None else (C.c_uint32 * len(classes))(*classes)
        rc, text = answer(lib, lib.svr_region_seed_classes(xyz, cls, len(seeds) if n is None else n, dims, out))
        assert "svr_region_seed_classes" in text and (buf == 0x5A).all()
        return rc, text
    ok = [(1, 2, 3)]
    assert call(None, [1], n=1)[0] == -4 and call(ok, None)[0] == -4 and call(ok, [1], dims=None)[0] == -4 and call(ok, [1], out=None)[0] == -4
    rc, text = call(ok, [1], dims=(C.c_int32 * 3)(4, 0, 6))
    assert rc == -6 and "bad dimensions" in text
    rc, text = call([(1, 2, 3), (0, 0, 0)], [4, 0])
    assert rc == -3 and "class 0" in text and "seed 1" in text
    rc, text = call(ok, [1], n=0)
    assert rc == -3 and "nseeds" in text
    rc, text = call([(0, 0, 0)] * 65, [1] * 65)
    assert rc == -3 and "nseeds" in text and "65" in text
    for bad in ((4, 0, 0), (0, 5, 0), (0, 0, 6), (-1, 0, 0)):
        rc, text = call([(0, 0, 0), bad], [1, 2])
        assert rc == -3 and "outside" in text, bad


def test_label_paint_refusals(lib):
    buf = np.full(2048, 0x5A, np.uint8)
    labels, mask = buf.ctypes.data, buf.ctypes.data + 1024
    dims = (C.c_int32 * 3)(4, 4, 4)

    def call(labels=labels, dims=dims, mask=mask, label=1):
        rc, text = answer(lib, lib.svr_region_label_paint(None if labels is None else C.c_void_p(labels), dims, None if mask is None else C.c_void_p(mask), label, 0))
        assert "svr_region_label_paint" in text and (buf == 0x5A).all()
        return rc, text
    assert call(labels=None)[0] == -4 and call(dims=None)[0] == -4 and call(mask=None)[0] == -4
    rc, text = call(dims=(C.c_int32 * 3)(4, 4, -4))
    assert rc == -6 and "bad dimensions" in text
    rc, text = call(label=0)
    assert rc == -3 and "non-zero" in text
    rc, text = call(mask=labels + 252)
    assert rc == -3 and "must not overlap" in text


def test_timer_refusal(lib):
    rc, text = answer(lib, lib.svr_region_growcut_last_ms(None))
    assert rc == -4 and "svr_region_growcut_last_ms" in text
