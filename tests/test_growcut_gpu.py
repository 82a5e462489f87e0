"""svr_region_growcut / _seed_classes / _label_paint on the GPU, through the raw C ABI on buffers the test owns: every cost and zones array
is EQUAL to the test-side reference (tests/growcut_ref.py: the Jacobi iteration on packed keys with the image term and the saturating
add).  Output buffers are pre-filled with a pattern.  The shapes are the smallest at which tiles and halos can go wrong; the fixtures
and the conditions they meet are those of tests/test_growcut_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import distance_ref as dr
from tests import geodesic_ref as gr
from tests import growcut_ref as gc
from tests import label_ref as lr
from tests import morph_ref as mr
from tests import region_ref as rr
from tests.test_distance_gpu import same_map, same_mask
from tests.test_geodesic_gpu import Geo, same_pair

pytestmark = pytest.mark.gpu


class Grow(Geo):
    """Raw grow-from-seeds calls on buffers the test owns."""

    def dims3(self):
        return (C.c_int32 * 3)(*self.dims)

    def params(self, weights, gain, shift, max_sweeps=0):
        p = abi.GrowcutParams()
        p.step_weights[:] = [int(w) for w in weights]
        p.contrast_gain, p.contrast_shift, p.max_sweeps = gain, shift, max_sweeps
        return p

    def growcut_rc(self, vox, labels, domain, weights, gain, shift, cost, zones, max_sweeps=0, on_dev=1):
        """(return code, error text, info); vox is a device pointer, or a host array with on_dev = 0."""
        info = abi.GrowcutInfo()
        src = C.c_void_p(vox) if on_dev else vox.ctypes.data_as(C.c_void_p)
        p = self.params(weights, gain, shift, max_sweeps)
        rc = self.lib.svr_region_growcut(src, self.dims3(), on_dev, C.c_void_p(labels), None if domain is None else C.c_void_p(domain), C.byref(p),
                                         None if cost is None else C.c_void_p(cost), None if zones is None else C.c_void_p(zones), C.byref(info))
        rc, msg = self.rc(rc)
        return rc, msg, info

    def growcut(self, vox, labels, domain, weights, gain, shift, cost, zones, **kw):
        """(cost, zones, info) as host arrays (None for a NULL output)."""
        rc, msg, info = self.growcut_rc(vox, labels, domain, weights, gain, shift, cost, zones, **kw)
        assert rc == 0, msg
        return None if cost is None else self.get_map(cost), None if zones is None else self.get_map(zones), info

    def put_domain(self, domain, padding=True):
        """The device mask of a bool array with garbage in the padding bits, or None."""
        if domain is None:
            return None
        words = rr.pack(domain)
        return self.put(mr.dirty_padding(words, self.shape) if padding else words)


def unreached(want, domain):
    return int((want[0] == gc.NONE).sum()) if domain is None else int((domain & (want[0] == gc.NONE)).sum())


def run_combinations(hip_dev, shape):
    with Grow(hip_dev, shape) as g:
        cap = hip_dev.lib.svr_region_geodesic_default_max_sweeps(*g.dims)
        uploaded = {}
        for kind, density, name, gs in gc.combinations(shape):
            vox, labels, domain = gc.case(shape, kind, density)
            if (kind, density) not in uploaded:
                uploaded[kind, density] = (g.put(vox), g.put(labels), g.put_domain(domain))
            v, lab, dom = uploaded[kind, density]
            want = gc.cached_case(shape, kind, density, name, gs)
            cost, zones, info = g.growcut(v, lab, dom, gc.WEIGHT_SETS[name], *gs, g.map(), g.map())
            same_pair((cost, zones), want, (shape, kind, density, name, gs))
            assert (info.unreached, info.saturated) == (unreached(want, domain), 0) and 1 <= info.sweeps <= cap
        for (kind, density), (v, lab, dom) in uploaded.items():                           # the inputs are not written
            vox, labels, _ = gc.case(shape, kind, density)
            assert np.array_equal(hip_dev.to_host(v, shape, np.uint16), vox) and np.array_equal(g.get_map(lab), labels)


# ------------------------------------------------------------------------------------------------ random volumes, domains and parameters
@pytest.mark.parametrize("shape", gc.TILED_SHAPES + [gc.ONE_TILE], ids=str)
def test_tiled_shapes(hip_dev, shape):
    run_combinations(hip_dev, shape)


@pytest.mark.parametrize("shape", gr.FLAT_SHAPES, ids=str)
def test_flat_shapes(hip_dev, shape):
    run_combinations(hip_dev, shape)


@pytest.mark.parametrize("density", gr.DENSITIES)
def test_gain_zero_equals_the_geodesic_call(hip_dev, density):
    shape = gc.TILED_SHAPES[1]
    vox, labels, domain = gc.case(shape, "full", density)
    with Grow(hip_dev, shape) as g:
        v, lab, dom = g.put(vox), g.put(labels), g.put_domain(domain)
        for name, w in gc.WEIGHT_SETS.items():
            geo = g.geodesic(lab, dom, w, g.map(), g.map())
            for shift in (0, 5):
                cost, zones, info = g.growcut(v, lab, dom, w, 0, shift, g.map(), g.map())
                same_pair((cost, zones), geo[:2], (density, name, shift))
            assert info.unreached == int((domain & (geo[0] == gc.NONE)).sum())


# ------------------------------------------------------------------------------------------------ saturation
def test_saturation_is_flagged_and_defined(hip_dev):
    w = gc.default_weights(6)
    for swapped in (False, True):
        vox, labels = gc.saturating_line(swapped)
        want = gc.growcut(vox, labels, None, w, gc.SAT_GAIN, 0)
        with Grow(hip_dev, gc.SAT_SHAPE) as g:
            cost, zones = g.map(), g.map()
            rc, msg, info = g.growcut_rc(g.put(vox), g.put(labels), None, w, gc.SAT_GAIN, 0, cost, zones)
            assert rc == abi.REGION_ERR_RANGE == -12 and "svr_region_growcut" in msg and "contrast_shift" in msg and "contrast_gain" in msg
            assert info.saturated == int((want[0] == gc.CAP).sum()) == gc.SAT_SHAPE[2] - 6 and info.unreached == 0 and info.sweeps >= 1
            got = (g.get_map(cost), g.get_map(zones))
            same_pair(got, want, ("saturated line", swapped))
            plateau = got[0] == gc.CAP
            assert plateau.any() and (got[1][plateau] == 3).all()                         # the smaller label of the two end seeds
            # one shift more and nothing saturates
            cost, zones, info = g.growcut(g.put(vox), g.put(labels), None, w, gc.SAT_GAIN, 8, g.map(), g.map())
            same_pair((cost, zones), gc.growcut(vox, labels, None, w, gc.SAT_GAIN, 8), "shift 8")
            assert info.saturated == 0


def test_saturation_across_tiles(hip_dev):
    """A checkerboard of 0 / 65535 under 6-moves: every move crosses full contrast, so the plateau spans all tiles and the labels travel
    over it from tile to tile."""
    shape = gc.TILED_SHAPES[0]
    vox = (np.indices(shape).sum(axis=0) % 2 * 65535).astype(np.uint16)
    _, labels, domain = gc.case(shape, "full", 0.7)
    w = gc.default_weights(6)
    want = gr.cached(("growcut", "checkerboard"), lambda: gc.growcut(vox, labels, domain, w, 30000, 0))
    assert (want[0] == gc.CAP).sum() > 100 and len(np.unique(want[1][want[0] == gc.CAP])) >= 2
    with Grow(hip_dev, shape) as g:
        cost, zones = g.map(), g.map()
        rc, msg, info = g.growcut_rc(g.put(vox), g.put(labels), g.put_domain(domain), w, 30000, 0, cost, zones)
        assert rc == abi.REGION_ERR_RANGE, msg
        same_pair((g.get_map(cost), g.get_map(zones)), want, "checkerboard")
        assert info.saturated == int((want[0] == gc.CAP).sum()) and info.unreached == unreached(want, domain)


# ------------------------------------------------------------------------------------------------ sources, outputs, aliases
def test_host_source_null_outputs_and_in_place(hip_dev):
    shape = gc.TILED_SHAPES[0]
    kind, density, name, gs = "full", 0.45, "anisotropic", (7, 3)
    vox, labels, domain = gc.case(shape, kind, density)
    want = gc.cached_case(shape, kind, density, name, gs)
    w = gc.WEIGHT_SETS[name]
    assert (domain & (want[0] == gc.NONE)).any()                                          # pockets that no marker reaches
    with Grow(hip_dev, shape) as g:
        lab, dom = g.put(labels), g.put_domain(domain)
        cost, zones, info = g.growcut(np.ascontiguousarray(vox), lab, dom, w, *gs, g.map(), g.map(), on_dev=0)
        same_pair((cost, zones), want, "host source")
        assert info.unreached == unreached(want, domain)
        same_pair(g.growcut(g.put(vox), lab, g.put_domain(domain, padding=False), w, *gs, g.map(), g.map())[:2], want, "clean padding")
        v = g.put(vox)
        cost, none, _ = g.growcut(v, lab, dom, w, *gs, g.map(), None)
        assert none is None
        same_map(cost, want[0], "zones NULL")
        none, zones, _ = g.growcut(v, lab, dom, w, *gs, None, g.map())
        assert none is None
        same_map(zones, want[1], "cost NULL")
        cost, zones, _ = g.growcut(v, lab, dom, w, *gs, g.map(), lab)                      # zones written over the markers
        same_pair((cost, zones), want, "in place")


def test_no_source_at_all(hip_dev):
    shape = gc.TILED_SHAPES[0]
    vox, labels, domain = gc.case(shape, "small", 0.7)
    with Grow(hip_dev, shape) as g:
        v = g.put(vox)
        for lab, dom in ((np.zeros_like(labels), None), (np.zeros_like(labels), domain), (np.where(domain, 0, labels).astype(np.uint32), domain)):
            cost, zones, info = g.growcut(v, g.put(lab), g.put_domain(dom), gc.default_weights(26), 1, 0, g.map(), g.map())
            assert (cost == gc.NONE).all() and not zones.any()
            assert info.unreached == (vox.size if dom is None else int(dom.sum())) and info.saturated == 0


def test_serpentine_completes_under_the_default_cap(hip_dev):
    labels, domain = gr.serpentine()
    want = gr.cached_geodesic("serpentine", labels, domain)                                # a constant image adds nothing to a move
    vox = np.full(gr.SERPENTINE_SHAPE, 1000, dtype=np.uint16)
    with Grow(hip_dev, gr.SERPENTINE_SHAPE) as g:
        v, lab, dom = g.put(vox), g.put(labels), g.put_domain(domain)
        cost, zones, info = g.growcut(v, lab, dom, gr.CHAMFER, 1, 0, g.map(), g.map())
        same_pair((cost, zones), want, "serpentine")
        cap = hip_dev.lib.svr_region_geodesic_default_max_sweeps(*g.dims)
        print(f"serpentine: {info.sweeps} sweeps, default cap {cap}")
        assert 3 <= info.sweeps <= cap and int(cost[domain].max()) == gr.SERPENTINE_MAX
        rc, msg, info = g.growcut_rc(v, lab, dom, gr.CHAMFER, 1, 0, g.map(), g.map(), max_sweeps=1)
        assert rc == abi.REGION_ERR_SWEEPS and info.sweeps == 1 and "svr_region_growcut" in msg


# ------------------------------------------------------------------------------------------------ markers
def test_seed_classes(hip_dev):
    shape = gc.TILED_SHAPES[1]
    nz, ny, nx = shape
    seeds = [(nx - 1, ny - 1, nz - 1), (0, 0, 0), (33, 8, 8), (0, 0, 0), (33, 8, 8), (5, 6, 7)]
    classes = [2, 1, 0xFFFFFFFF, 3, 1, 2]
    want = gc.seed_classes(seeds, classes, shape)
    assert want[0, 0, 0] == 1 and want[8, 8, 33] == 0xFFFFFFFF
    with Grow(hip_dev, shape) as g:
        out = g.map()
        xyz = (C.c_int32 * (3 * len(seeds)))(*[c for s in seeds for c in s])
        g.ok(g.lib.svr_region_seed_classes(xyz, (C.c_uint32 * len(classes))(*classes), len(seeds), g.dims3(), C.c_void_p(out)))
        hip_dev.synchronize()
        same_map(g.get_map(out), want, "seed classes")
    assert np.array_equal(hip_dev.region_seed_classes(seeds, classes, shape), want)


def test_label_paint(hip_dev):
    shape = gc.TILED_SHAPES[0]
    labels = gc.class_markers(shape, 300, 5)
    mask = gr.random_domain(shape, 0.3, 6)
    assert (mask & (labels != 0)).any() and (mask & (labels == 0)).any()
    with Grow(hip_dev, shape) as g:
        words = g.put(mr.dirty_padding(rr.pack(mask), shape))
        for only in (0, 1):
            lab = g.put(labels)
            g.ok(g.lib.svr_region_label_paint(C.c_void_p(lab), g.dims3(), C.c_void_p(words), 9, only))
            hip_dev.synchronize()
            same_map(g.get_map(lab), gc.label_paint(labels, mask, 9, bool(only)), ("label paint", only))
    assert np.array_equal(hip_dev.region_label_paint(labels, mask, 9, True), gc.label_paint(labels, mask, 9, True))


# ------------------------------------------------------------------------------------------------ the head: strokes, classes, the chain
def head_case():
    vox = scenes.make_ct_head_volume(gc.HEAD_N)
    return vox, gc.head_seeds(vox)


def head_markers_ref(vox, seeds):
    labels = np.zeros(vox.shape, dtype=np.uint32)
    for x, y, z, cls in seeds:
        point = np.zeros(vox.shape, dtype=bool)
        point[z, y, x] = True
        labels = gc.label_paint(labels, dr.ball(point, dr.DILATE, gc.HEAD_R2), cls, True)
    return labels


def test_head_strokes_classes_and_the_chain(hip_dev):
    vox, seeds = head_case()
    shape = vox.shape
    markers = gr.cached(("growcut", "head markers"), lambda: head_markers_ref(vox, seeds))
    w = gc.default_weights(6)
    want = gr.cached(("growcut", "head"), lambda: gc.growcut(vox, markers, None, w, 1, 4))
    counts = np.bincount(want[1].reshape(-1), minlength=4)
    assert counts[0] == 0 and (counts[1:4] > 500).all()                                   # every class owns a real part of the volume
    with Grow(hip_dev, shape) as g:
        lab = g.raw(4 * g.n, prefill=0)
        for x, y, z, cls in seeds:                                                        # a stroke: the seed's voxel, a ball around it, painted
            point = np.zeros(shape, dtype=bool)
            point[z, y, x] = True
            stroke = g.raw(4 * g.words)
            g.ok(g.lib.svr_region_ball(C.c_void_p(g.put(rr.pack(point))), *g.dims, abi.MORPH_DILATE, None, gc.HEAD_R2, C.c_void_p(stroke)))
            g.ok(g.lib.svr_region_label_paint(C.c_void_p(lab), g.dims3(), C.c_void_p(stroke), cls, 1))
        hip_dev.synchronize()
        same_map(g.get_map(lab), markers, "head markers")
        cost, zones, info = g.growcut(g.put(vox), lab, None, w, 1, 4, g.map(), lab)        # the zones replace the markers
        same_pair((cost, zones), want, "head")
        assert (info.unreached, info.saturated) == (0, 0)
        bone = gc.HEAD_CLASSES["bone"]
        keep = np.zeros(4, dtype=np.uint8)
        keep[bone] = 1
        same_mask(g.select(lab, 3, keep, g.raw(4 * g.words)), want[1] == bone, "select bone")
        table = hip_dev.region_label_table(lab, 3, shape=shape)
        want_table = lr.table(want[1], 3)
        for field in ("voxels", "first", "bbox_min", "bbox_max"):
            assert np.array_equal(table[field], want_table[field]), field
        assert int(table["voxels"][bone - 1]) == int(counts[bone])


# ------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_and_timer(hip_dev):
    shape = gc.TILED_SHAPES[0]
    kind, density, name, gs = "small", 0.7, "26", (1, 0)
    vox, labels, domain = gc.case(shape, kind, density)
    want = gc.cached_case(shape, kind, density, name, gs)
    cost, zones, info = hip_dev.region_growcut(vox, labels, domain)
    same_pair((cost, zones), want, "Device.region_growcut")
    assert info.sweeps >= 1 and info.unreached == unreached(want, domain) and hip_dev.region_growcut_last_ms() > 0.0
    cost, zones, _ = hip_dev.region_growcut(vox, labels, domain, want_zones=False)
    assert zones is None and np.array_equal(cost, want[0])
    want = gc.cached_case(shape, "small", None, "anisotropic", (7, 3))
    vox, labels, _ = gc.case(shape, "small", None)
    cost, zones, _ = hip_dev.region_growcut(vox, labels, step_weights=gc.WEIGHT_SETS["anisotropic"], gain=7, shift=3, want_cost=False)
    assert cost is None and np.array_equal(zones, want[1])
    vox, labels = gc.saturating_line()
    with pytest.raises(host.SvrError) as err:
        hip_dev.region_growcut(vox, labels, connectivity=6, gain=gc.SAT_GAIN)
    assert err.value.code == abi.REGION_ERR_RANGE and err.value.info.saturated == gc.SAT_SHAPE[2] - 6
    same_pair((err.value.cost, err.value.zones), gc.growcut(vox, labels, None, gc.default_weights(6), gc.SAT_GAIN, 0), "saturated, Python layer")
