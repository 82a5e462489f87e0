"""svr_region_geodesic / _seed_labels / _split / _zone_cut on the GPU, through the raw C ABI on buffers the test owns: every dist and zones
array and every mask -- as uint32 words, padding included -- is EQUAL to the test-side reference (tests/geodesic_ref.py: the Jacobi iteration
on packed keys).  Output buffers are pre-filled with a pattern.  The fixtures and the conditions they meet are those of
tests/test_geodesic_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import distance_ref as dr
from tests import geodesic_ref as gr
from tests import label_ref as lr
from tests import morph_ref as mr
from tests import region_ref as rr
from tests.test_distance_gpu import same_map, same_mask

pytestmark = pytest.mark.gpu


class Geo:
    """Raw calls on buffers the test owns."""

    def __init__(self, dev, shape):
        self.dev, self.lib, self.shape = dev, dev.lib, tuple(shape)
        self.dims = (shape[2], shape[1], shape[0])
        self.words = host.region_mask_words(shape)
        self.n = int(np.prod(shape))
        self.bufs = []

    def raw(self, nbytes, prefill=0xA5):
        p = self.dev.malloc(max(nbytes, 4))
        self.bufs.append(p)
        self.dev.check(self.lib.svr_memset_device(C.c_void_p(p), prefill, max(nbytes, 4)))       # the calls overwrite whatever is there
        return p

    def put(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.raw(a.nbytes)
        self.dev.to_device(p, a)
        return p

    def map(self):
        return self.raw(4 * self.n)

    def rc(self, rc):
        msg = self.lib.svr_last_error().decode()
        self.lib.svr_clear_error()
        return rc, msg

    def ok(self, rc):
        rc, msg = self.rc(rc)
        assert rc == 0, msg

    def get_map(self, p):
        return self.dev.to_host(p, self.shape, np.uint32)

    def get_mask(self, p):
        self.dev.synchronize()
        return self.dev.to_host(p, (self.words,), np.uint32)

    @staticmethod
    def w7(weights):
        return None if weights is None else (C.c_uint32 * 7)(*weights)

    def geodesic_rc(self, labels, domain, weights, dist, zones, max_sweeps=0):
        sweeps = C.c_uint32(0xFFFFFFFF)
        rc = self.lib.svr_region_geodesic(C.c_void_p(labels), C.c_void_p(domain), *self.dims, self.w7(weights), max_sweeps,
                                          None if dist is None else C.c_void_p(dist), None if zones is None else C.c_void_p(zones), C.byref(sweeps))
        return rc, int(sweeps.value)

    def geodesic(self, labels, domain, weights, dist, zones, max_sweeps=0):
        """(dist, zones, sweeps) as host arrays (None for a NULL output)."""
        rc, sweeps = self.geodesic_rc(labels, domain, weights, dist, zones, max_sweeps)
        self.ok(rc)
        return None if dist is None else self.get_map(dist), None if zones is None else self.get_map(zones), sweeps

    def run(self, labels, domain, weights=gr.CHAMFER, padding=False):
        """Uploads a case and runs it into fresh buffers: (dist, zones, sweeps)."""
        words = rr.pack(domain)
        if padding:
            words = mr.dirty_padding(words, self.shape)
        return self.geodesic(self.put(labels), self.put(words), weights, self.map(), self.map())

    def split(self, mask_ptr, r2, connectivity, steps, zones, dist_weights=None, max_sweeps=0):
        count, lost, sweeps = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF)
        dw = None if dist_weights is None else (C.c_uint32 * 3)(*dist_weights)
        self.ok(self.lib.svr_region_split(C.c_void_p(mask_ptr), *self.dims, dw, r2, connectivity, self.w7(steps), max_sweeps, C.c_void_p(zones),
                                          C.byref(count), C.byref(lost), C.byref(sweeps)))
        return self.get_map(zones), int(count.value), int(lost.value), int(sweeps.value)

    def zone_cut(self, zones_ptr, connectivity, out):
        self.ok(self.lib.svr_region_zone_cut(C.c_void_p(zones_ptr), *self.dims, connectivity, C.c_void_p(out)))
        return self.get_mask(out)

    def label(self, mask_ptr, connectivity, out):
        k = C.c_uint32(0xFFFFFFFF)
        self.ok(self.lib.svr_region_label(C.c_void_p(mask_ptr), *self.dims, connectivity, C.c_void_p(out), C.byref(k)))
        return self.get_map(out), int(k.value)

    def select(self, labels_ptr, count, keep, out):
        self.ok(self.lib.svr_region_select(C.c_void_p(labels_ptr), *self.dims, count, C.c_void_p(self.put(np.asarray(keep, dtype=np.uint8))), C.c_void_p(out)))
        return self.get_mask(out)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.dev.free(p)
        self.bufs = []


def same_pair(got, want, what):
    same_map(got[0], want[0], (what, "dist"))
    same_map(got[1], want[1], (what, "zones"))


# ------------------------------------------------------------------------------------------------ random domains
@pytest.mark.parametrize("density", gr.DENSITIES)
def test_random_domains_all_weight_sets(hip_dev, density):
    domain, labels = gr.random_case(density)
    with Geo(hip_dev, gr.GPU_SHAPE) as g:
        lab, dom = g.put(labels), g.put(rr.pack(domain))
        for name, w in gr.WEIGHT_SETS.items():
            want = gr.cached_geodesic(f"random {density}", labels, domain, w)
            first = g.geodesic(lab, dom, w, g.map(), g.map())
            same_pair(first, want, (density, name))
            assert 1 <= first[2] <= hip_dev.lib.svr_region_geodesic_default_max_sweeps(*g.dims)
            again = g.geodesic(lab, dom, w, g.map(), g.map())                              # once more into fresh buffers
            same_pair(again, first, (density, name, "second run"))
        assert np.array_equal(g.get_map(lab), labels)                                     # the inputs are not written


def test_null_weights_are_the_chamfer_weights(hip_dev):
    domain, labels = gr.random_case(0.7)
    with Geo(hip_dev, gr.GPU_SHAPE) as g:
        same_pair(g.run(labels, domain, None), gr.cached_geodesic("random 0.7", labels, domain, gr.CHAMFER), "NULL weights")


def test_padding_null_outputs_and_in_place(hip_dev):
    domain, labels = gr.random_case(0.45)
    want = gr.cached_geodesic("random 0.45", labels, domain, gr.CHAMFER)
    assert (domain & (want[0] == gr.NONE)).any()                                          # pockets that no marker reaches
    with Geo(hip_dev, gr.GPU_SHAPE) as g:
        same_pair(g.run(labels, domain, padding=True), want, "input padding bits set")
        lab, dom = g.put(labels), g.put(rr.pack(domain))
        dist, none, _ = g.geodesic(lab, dom, gr.CHAMFER, g.map(), None)
        assert none is None
        same_map(dist, want[0], "zones NULL")
        none, zones, _ = g.geodesic(lab, dom, gr.CHAMFER, None, g.map())
        assert none is None
        same_map(zones, want[1], "dist NULL")
        dist, zones, _ = g.geodesic(lab, dom, gr.CHAMFER, g.map(), lab)                    # zones written over the labels
        same_pair((dist, zones), want, "in place")


def test_no_source_at_all(hip_dev):
    domain, labels = gr.random_case(0.7)
    with Geo(hip_dev, gr.GPU_SHAPE) as g:
        for lab in (np.zeros_like(labels), np.where(domain, 0, labels).astype(np.uint32)):     # no label; labels only outside the domain
            dist, zones, _ = g.run(lab, domain)
            assert (dist == gr.NONE).all() and not zones.any()


# ------------------------------------------------------------------------------------------------ flat and tiny shapes
@pytest.mark.parametrize("shape", gr.FLAT_SHAPES, ids=str)
def test_flat_shapes(hip_dev, shape):
    domain = gr.random_domain(shape, 0.8, 3)
    labels = gr.random_markers(shape, 3, 4)
    full = np.ones(shape, dtype=bool)
    corner = np.zeros(shape, dtype=np.uint32)
    corner[0, 0, 0] = 0xFFFFFFFF
    with Geo(hip_dev, shape) as g:
        for name, w in gr.WEIGHT_SETS.items():
            same_pair(g.run(labels, domain, w), gr.geodesic(labels, domain, w), (shape, name))
        dist, zones, _ = g.run(corner, full)                                              # a full row: the distance is 3 per step
        want = 3 * np.arange(full.size, dtype=np.uint32).reshape(shape)
        same_pair((dist, zones), (want, np.full(shape, 0xFFFFFFFF, dtype=np.uint32)), (shape, "row"))


# ------------------------------------------------------------------------------------------------ a source on a tile face
# A source never falls, so its tile's block marks no neighbour tile for it: the init kernel has to wake the tile across the face.  The
# smallest shapes at which that can go wrong: one marker on either side of the first tile face of each axis, in a domain that has no
# other voxel on the face layer.  (shape, domain voxels or None = all, marker (z, y, x), label, the line's distances or its last four)
_DIAGONAL = [(6 + k, 6 + k, 30 + k) for k in range(4)]
FACE_CASES = [
    ((1, 1, 34), None, (0, 0, 31), 5, [3, 0, 3, 6]),
    ((1, 1, 34), None, (0, 0, 32), 5, [6, 3, 0, 3]),
    ((1, 10, 1), None, (0, 7, 0), 5, [3, 0, 3, 6]),
    ((1, 10, 1), None, (0, 8, 0), 5, [6, 3, 0, 3]),
    ((10, 1, 1), None, (7, 0, 0), 5, [3, 0, 3, 6]),
    ((10, 1, 1), None, (8, 0, 0), 5, [6, 3, 0, 3]),
    ((10, 10, 34), _DIAGONAL, (7, 7, 31), 9, [5, 0, 5, 10]),
    ((10, 10, 34), _DIAGONAL, (8, 8, 32), 9, [10, 5, 0, 5]),
]


@pytest.mark.parametrize("shape, voxels, marker, label, line", FACE_CASES, ids=[f"{c[0]}-{c[2]}".replace(" ", "") for c in FACE_CASES])
def test_source_on_a_tile_face(hip_dev, shape, voxels, marker, label, line):
    from tests.test_growcut_gpu import Grow                                               # (that module imports this one)

    domain = np.ones(shape, dtype=bool)
    if voxels is not None:
        domain[:] = False
        domain[tuple(zip(*voxels))] = True
    labels = np.zeros(shape, dtype=np.uint32)
    labels[marker] = label
    want = gr.geodesic(labels, domain)
    assert want[0][domain][-4:].tolist() == line and (want[1][domain] == label).all()     # the reference, by hand
    with Grow(hip_dev, shape) as g:
        lab, dom = g.put(labels), g.put(rr.pack(domain))
        dist, zones, _ = g.geodesic(lab, dom, gr.CHAMFER, g.map(), g.map())
        same_pair((dist, zones), want, (shape, marker))
        cost, zones, info = g.growcut(g.put(np.full(shape, 1000, dtype=np.uint16)), lab, dom, gr.CHAMFER, 0, 0, g.map(), g.map())
        same_pair((cost, zones), want, (shape, marker, "growcut, gain 0"))
        assert (info.unreached, info.saturated) == (0, 0)


def test_split_core_on_a_tile_face(hip_dev):
    """Two cores, one of them the three voxels from the last one of the first tile on.  (With r2 = 0 every voxel of the mask is a core
    voxel, so nothing has to cross the face: a pin, which the init kernel that marked only a source's own tile passed as well.)"""
    shape = (1, 1, 34)
    m = np.ones(shape, dtype=bool)
    m[0, 0, 30] = False
    want, want_count, want_lost = gr.split(m, 0, 6)
    assert (want_count, want_lost) == (2, 0) and want[0, 0, 29:].tolist() == [1, 0, 2, 2, 2]
    with Geo(hip_dev, shape) as g:
        zones, count, lost, _ = g.split(g.put(rr.pack(m)), 0, 6, None, g.map())
        same_map(zones, want, "split on a face")
        assert (count, lost) == (want_count, 0)


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("axis, middle", gr.TIE_CASES)
def test_ties_go_to_the_smaller_label(hip_dev, axis, middle):
    with Geo(hip_dev, gr.GPU_SHAPE) as g:
        for swapped in (False, True):
            labels, domain, mid = gr.tie_line(axis, middle, swapped)
            dist, zones, _ = g.run(labels, domain)
            assert zones[mid] == 3 and dist[mid] == 15
            same_pair((dist, zones), gr.geodesic(labels, domain), (axis, middle, swapped))


# ------------------------------------------------------------------------------------------------ the serpentine and the sweep cap
def test_serpentine_completes_under_the_default_cap(hip_dev):
    labels, domain = gr.serpentine()
    want = gr.cached_geodesic("serpentine", labels, domain)
    with Geo(hip_dev, gr.SERPENTINE_SHAPE) as g:
        dist, zones, sweeps = g.run(labels, domain)
        same_pair((dist, zones), want, "serpentine")
        assert int(dist[domain].max()) == gr.SERPENTINE_MAX
        print(f"serpentine: {sweeps} sweeps, default cap {hip_dev.lib.svr_region_geodesic_default_max_sweeps(*g.dims)}")
        assert 3 <= sweeps <= hip_dev.lib.svr_region_geodesic_default_max_sweeps(*g.dims)
        rc, sweeps = g.geodesic_rc(g.put(labels), g.put(rr.pack(domain)), gr.CHAMFER, g.map(), g.map(), max_sweeps=1)
        rc, msg = g.rc(rc)
        assert rc == abi.REGION_ERR_SWEEPS and sweeps == 1 and "svr_region_geodesic" in msg


# ------------------------------------------------------------------------------------------------ seed labels
def test_seed_labels(hip_dev):
    shape = gr.GPU_SHAPE
    nz, ny, nx = shape
    seeds = [(nx - 1, ny - 1, nz - 1), (0, 0, 0), (33, 8, 8), (0, 0, 0), (33, 8, 8), (5, 6, 7)]
    with Geo(hip_dev, shape) as g:
        out = g.map()
        xyz = (C.c_int32 * (3 * len(seeds)))(*[c for s in seeds for c in s])
        g.ok(g.lib.svr_region_seed_labels(xyz, len(seeds), *g.dims, C.c_void_p(out)))
        hip_dev.synchronize()
        same_map(g.get_map(out), gr.seed_labels(seeds, shape), "seed labels")
    assert np.array_equal(hip_dev.region_seed_labels(seeds, shape), gr.seed_labels(seeds, shape))


# ------------------------------------------------------------------------------------------------ split, cut, label table
def test_split_phantom_zone_cut_and_label_table(hip_dev):
    m = gr.two_ball_phantom()
    with Geo(hip_dev, gr.PHANTOM_SHAPE) as g:
        src = g.put(mr.dirty_padding(rr.pack(m), g.shape))
        _, k = g.label(src, 26, g.map())
        assert k == 1
        for name, steps, conn in (("chamfer", None, 26), ("6", gr.PHANTOM_6_WEIGHTS, 26)):
            want, want_count, want_lost = gr.split(m, gr.PHANTOM_R2, conn, step_weights=steps)
            zptr = g.map()
            zones, count, lost, sweeps = g.split(src, gr.PHANTOM_R2, conn, steps, zptr)
            same_map(zones, want, ("split", name))
            assert (count, lost) == (want_count, want_lost) == (2, 0) and sweeps >= 1
            assert tuple(np.bincount(zones.reshape(-1))[1:].tolist()) == gr.PHANTOM_ZONES[name]
            move_conn = 26 if steps is None else 6
            for zone in (1, 2):                                                           # an influence zone is connected under the moves
                keep = np.zeros(count + 1, dtype=np.uint8)
                keep[zone] = 1
                part = g.select(zptr, count, keep, g.raw(4 * g.words))
                same_mask(part, want == zone, ("select", name, zone))
                assert g.label(g.put(part), move_conn, g.map())[1] == 1, (name, zone)
            for cut_conn in lr.CONNS:
                cut = g.zone_cut(zptr, cut_conn, g.raw(4 * g.words))
                same_mask(cut, gr.zone_cut(want, cut_conn), ("zone cut", name, cut_conn))
                assert g.label(g.put(cut), cut_conn, g.map())[1] == 2                     # two parts where the mask was one
            table = hip_dev.region_label_table(zptr, count, shape=g.shape)
            assert tuple(int(t) for t in table["voxels"]) == gr.PHANTOM_ZONES[name]
            want_table = lr.table(want, count)                                            # zones change label inside a run of set voxels
            for field in ("voxels", "first", "bbox_min", "bbox_max"):
                assert np.array_equal(table[field], want_table[field]), (name, field)
        # the Python layer
        zones, count, lost, _ = hip_dev.region_split(m, gr.PHANTOM_R2, 26)
        assert np.array_equal(zones, gr.split(m, gr.PHANTOM_R2, 26)[0]) and (count, lost) == (2, 0)
        assert np.array_equal(hip_dev.region_zone_cut(zones, 26), gr.zone_cut(zones, 26))
        # a ball too large for any core: no part, everything unreached
        zones, count, lost, _ = g.split(src, gr.PHANTOM_R2_NONE, 26, None, g.map())
        assert count == 0 and not zones.any() and lost == m.sum()


def test_split_mask_with_thin_pieces(hip_dev):
    """Several cores under 18-moves and anisotropic distance weights, and pieces too thin to hold one (unreached > 0)."""
    m = gr.thin_pieces_mask()
    want, want_count, want_lost = gr.cached(("thin",), lambda: gr.split(m, gr.THIN_R2, 18, dist_weights=gr.THIN_DIST_WEIGHTS))
    assert want_count >= 2 and 0 < want_lost < m.sum()
    with Geo(hip_dev, gr.GPU_SHAPE) as g:
        zones, count, lost, _ = g.split(g.put(rr.pack(m)), gr.THIN_R2, 18, None, g.map(), dist_weights=gr.THIN_DIST_WEIGHTS)
        same_map(zones, want, "split 18")
        assert (count, lost) == (want_count, want_lost)


def test_python_layer_geodesic_and_timer(hip_dev):
    domain, labels = gr.random_case(0.7)
    want = gr.cached_geodesic("random 0.7", labels, domain, gr.CHAMFER)
    dist, zones, sweeps = hip_dev.region_geodesic(labels, domain)
    same_pair((dist, zones), want, "Device.region_geodesic")
    assert sweeps >= 1 and hip_dev.region_geodesic_last_ms() > 0.0
    dist, zones, _ = hip_dev.region_geodesic(labels, domain, want_zones=False)
    assert zones is None and np.array_equal(dist, want[0])
