"""The shapes of the scale tests (tests/scale_ref.py) really cross the launch thresholds they are there for, the mirrored constants
are those of the sources, and the helpers that stand in for the literal references at millions of labels, or on sparse contents of very
large volumes, equal those references where both can run.  No device."""
import numpy as np
import pytest

from sunvolumerender_amd import abi, host
from tests import distance_ref as dr
from tests import label_ref as lr
from tests import mesh_ref as mr
from tests import morph_ref as mo
from tests import region_ref as rr
from tests import scale_ref as sr


# ------------------------------------------------------------------------------------------------ the mirrors
@pytest.mark.parametrize("name", sorted(sr.SOURCES))
def test_mirrors_equal_the_sources(name):
    values = sr.source_values(name)
    assert values, f"{name}: {sr.SOURCES[name][1]!r} no longer matches {sr.SOURCES[name][0]}"
    assert all(v == sr.MIRRORS[name] for v in values), (name, values, sr.MIRRORS[name])


def test_mirrors_that_the_package_keeps():
    assert sr.LABEL_SCAN_BLOCK == abi.LABEL_SCAN_BLOCK == host.LABEL_SCAN_BLOCK
    assert sr.REGION_WAVES == 4 and sr.REGION_TRIP == 8192 and sr.DISTANCE_MAX_TRIP == 524288 and sr.BBOX_TRIP == 65536


# ------------------------------------------------------------------------------------------------ the thresholds
# Each predicate says "this shape reaches the branch"; it holds for the shape of the tests and fails once the margin is taken away.
def second_region_trip(shape, vector):
    tasks = sr.region_tasks(shape, vector)
    return sr.REGION_TRIP < tasks < 2 * sr.REGION_TRIP                                   # a second trip, and a partial one


def second_grid_plane(rows, rows_per_block):
    groups, gy, gz = sr.row_grid(rows, rows_per_block)
    return gy == sr.GRID_Y_MAX and gz == 2 and groups % gy != 0                            # gridDim.z = 2, the last plane partly filled


@pytest.mark.parametrize("vector", [8, 1])
def test_region_shapes_take_a_second_partial_trip(vector):
    nz, ny, nx = shape = sr.REGION_SHAPES[vector]
    assert (nx % 8 == 0) == (vector == 8)                                                # the path the kernels take
    assert sr.region_tasks(shape, vector) == 9216 and second_region_trip(shape, vector)
    assert not second_region_trip((85, 96, nx), vector)                                  # 8 160 tasks: one trip
    assert not second_region_trip((nz, ny, 64 * vector + 1), vector)                     # two spans a row: 18 432 tasks, a full second trip
    vox, seeds, region, stats = sr.region_case(vector)
    rows = region.reshape(nz * ny, nx).any(axis=1)                                       # (one span a row: task = row)
    assert rows[:sr.REGION_TRIP].any() and rows[sr.REGION_TRIP:].any()                   # the region spans both trips
    assert 0.3 * vox.size < stats["voxels"] < vox.size and len(seeds) == 1


def test_filter_shape_needs_a_second_grid_plane():
    nz, ny, nx = sr.FILTER_SHAPE
    assert sr.row_grid(nz * ny, sr.SMOOTH_ROWS) == (65613, 65535, 2) and nz * ny == 524900 > 524280
    assert second_grid_plane(nz * ny, sr.SMOOTH_ROWS)
    assert not second_grid_plane(724 * 724, sr.SMOOTH_ROWS)
    assert sr.voxels(sr.FILTER_SHAPE) < 2_000_000
    # the rank kernels: tiles of 128 x 8 x 8, linear in blockIdx.x
    assert ((nx + 127) // 128) * ((ny + 7) // 8) * ((nz + 7) // 8) == 8281


@pytest.mark.parametrize("name", ["nearest", "linear", "area", "crop"])
def test_resample_output_needs_a_second_grid_plane(name):
    nz, ny, nx = sr.RESAMPLE_OUT
    assert sr.row_grid(nz * ny, sr.RESAMPLE_ROWS) == (65664, 65535, 2) and nz * ny == 262656 > 262140
    assert second_grid_plane(nz * ny, sr.RESAMPLE_ROWS)
    assert not second_grid_plane(511 * 512, sr.RESAMPLE_ROWS)
    grid = sr.resample_grid(name)
    from tests import resample_ref as rs
    from tests.test_resample_cpu import STEPS

    assert rs.grid_shape(grid) == sr.RESAMPLE_OUT
    src = sr.resample_source_shape(name)
    rs.check_grid(src[::-1], grid)
    assert sr.voxels(src) < 2_000_000
    if name == "crop":
        assert all(rs.is_copy(m) for m in grid)
    else:
        assert all(m[1] in STEPS and not rs.is_copy(m) for m in grid)


def test_distance_shape_takes_a_second_partial_trip():
    words, lanes = sr.mask_words(sr.DISTANCE_SHAPE), sr.lanes(sr.DISTANCE_SHAPE)
    assert words == 20480 > 16384 and sr.DISTANCE_MAX_TRIP < lanes == 655360 < 2 * sr.DISTANCE_MAX_TRIP
    assert not sr.DISTANCE_MAX_TRIP < sr.lanes((51, 64, 160))                            # 522 240 lanes: one trip
    assert sr.distance_lane(sr.DISTANCE_EARLY) < sr.DISTANCE_MAX_TRIP <= sr.distance_lane(sr.DISTANCE_LATE) < lanes
    m = sr.distance_map_noise()
    assert int(m[m != dr.NONE].max()) < sr.DISTANCE_PEAK and (m == dr.NONE).any()


def test_mesh_mask_has_more_vertices_than_one_trip():
    V, T, info = mr.mesh_region(sr.mesh_mask(), 0)
    assert sr.BBOX_TRIP < len(V) == info["vertices"] < 2 * sr.BBOX_TRIP, len(V)
    V, _, _ = mr.mesh_region(np.random.default_rng(73).random((30, 30, 30)) < 0.5, 0)
    assert len(V) < sr.BBOX_TRIP                                                         # a smaller mask stays within one


def test_label_shape_needs_four_scan_levels():
    assert sr.mask_words(sr.LABEL_SHAPE) == 16781312 > 1 << 24
    assert host.region_label_scan_levels(sr.LABEL_SHAPE) == 4
    assert host.region_label_scan_levels((4096, 4096, 1)) == 3
    assert sr.label_checker_count() == 8390656 > 1 << 23
    small = (5, 7, 1)
    assert int(sr.label_checker(small).sum()) == sr.label_checker_count(small) == lr.label(sr.label_checker(small), 6)[1] == 18


def test_narrow_shape_has_two_to_the_32_lanes():
    assert sr.mask_words(sr.NARROW_SHAPE) == 1 << 27 and sr.lanes(sr.NARROW_SHAPE) == 1 << 32
    assert sr.lanes((8192, 16383, 1)) < 1 << 32
    assert sr.voxels(sr.NARROW_SHAPE) == 1 << 27
    s = sr.Sparse(sr.NARROW_SHAPE, sr.narrow_points())
    rows = set(s.indices()[0].tolist())
    for row in (0, (1 << 26) - 1, 1 << 26, (1 << 27) - 1):
        assert row in rows
    assert len(set(s.points.values())) == len(s.points) and all(sr.NARROW_WINDOW[0] <= v <= sr.NARROW_WINDOW[1] for v in s.points.values())
    labelling, k = s.labels(6)
    assert k == 7 and len(set(labelling.values())) == 7
    assert s.labels(26)[1] == 7                                                          # rows 2^26 - 1 and 2^26 are no neighbours


@pytest.mark.parametrize("shape", [sr.L1, sr.L2], ids=["L1", "L2"])
def test_large_shapes_and_their_beacons(shape):
    n = sr.voxels(shape)
    assert n == (1 << 29 if shape == sr.L1 else 1 << 31)
    assert 4 * sr.voxels(sr.L1) == 1 << 31 and 8 * sr.voxels(sr.L1) == 1 << 32          # uint32 maps and 8-byte keys at L1
    assert 2 * sr.voxels(sr.L2) == 1 << 32 and 4 * sr.voxels(sr.L2) == 1 << 33          # u16 and uint32 maps at L2
    s = sr.Sparse(shape, sr.beacon_points(shape))
    idx, _ = s.indices()
    assert idx[0] == 0 and idx[-1] == n - 1                                              # the first and the last voxel
    for i in sr.plane_crossings(shape):
        near = idx[(idx >= i - 3 * shape[1] * shape[2]) & (idx < i + 3 * shape[1] * shape[2])]
        assert (near < i).any() and (near >= i).any(), i                                 # a beacon straddles the plane
    assert len(sr.plane_crossings(shape)) == (1 if shape == sr.L1 else 4)
    assert len(set(s.points.values())) == len(s.points)
    # a cut-out and a component for every beacon on its own and for every pair that a rod joins
    planes = len(sr.plane_crossings(shape))
    assert len(sr.beacon_origins(shape)) == 8 + 2 * planes + 2 and len(sr.beacon_rods(shape)) == planes + 2
    assert len(s.cutouts(3)) == sr.beacon_components(shape) == s.labels(6)[1] == s.labels(26)[1] == 8 + planes
    assert len(s.points) == 125 * len(sr.beacon_origins(shape)) + sr.ROD * len(sr.beacon_rods(shape))
    assert sr.hollow_centre(shape) in s.points


# ------------------------------------------------------------------------------------------------ the stand-ins equal the references
@pytest.mark.parametrize("conn", lr.CONNS)
def test_fast_label_helpers_equal_the_literal_ones(conn):
    for shape in ((9, 11, 1), (6, 7, 9)):
        m = lr.random_mask(shape, 0.45, 3)
        want, k = lr.label(m, conn)
        got, gk = sr.scipy_label(m, conn)
        assert gk == k and got.dtype == np.uint32 and np.array_equal(got, want)
        t, w = sr.fast_table(want, k), lr.table(want, k)
        for f in lr.COMPONENT_FIELDS:
            assert np.array_equal(t[f], w[f]) and t[f].dtype == w[f].dtype, f
        sizes = w["voxels"]
        for min_voxels, largest_k in ((0, 0), (2, 0), (0, 3), (2, 2), (1000, 0)):
            keep = sr.fast_kept(sizes, min_voxels, largest_k)
            assert np.flatnonzero(keep).tolist() == lr.kept_labels(sizes, min_voxels, largest_k)


def small_sparse():
    shape = (40, 37, 70)
    rng = np.random.default_rng(9)
    pts = {}
    for z0, y0, x0 in ((0, 0, 0), (20, 15, 30), (35, 32, 65), (19, 30, 2)):
        for dz, dy, dx in np.argwhere(rng.random((5, 5, 5)) < 0.6):
            pts[(z0 + int(dz), y0 + int(dy), x0 + int(dx))] = 100 + len(pts)
    for x in range(5, 30):
        pts[(22, 17, x)] = 100 + len(pts)
    s = sr.Sparse(shape, pts)
    dense = np.zeros(shape, dtype=np.uint16)
    for p, v in pts.items():
        dense[p] = v
    return s, dense


def test_sparse_helpers_equal_the_dense_references():
    s, dense = small_sparse()
    mask = dense > 0
    assert 1 < len(s.cutouts(3)) < 5
    idx, vals = s.indices()
    assert np.array_equal(idx, np.flatnonzero(dense)) and np.array_equal(vals, dense.reshape(-1)[idx])
    flat = np.zeros(dense.size, dtype=np.uint16)
    for at, run in s.x_runs():
        flat[at:at + len(run)] = run
    assert np.array_equal(flat.reshape(dense.shape), dense)
    widx, w = sr.sparse_words(s.shape, s.points)
    packed = rr.pack(mask)
    assert np.array_equal(np.flatnonzero(packed), widx) and np.array_equal(packed[widx], w)
    for conn in lr.CONNS:
        want, k = lr.label(mask, conn)
        labelling, gk = s.labels(conn)
        assert gk == k and all(want[p] == lab for p, lab in labelling.items())
        t, wt = s.table(labelling, k, s.points), lr.table(want, k, dense)
        for f in lr.COMPONENT_FIELDS:
            assert np.array_equal(t[f], wt[f]), f
    # the statistics of all points and of one component
    want, _ = lr.label(mask, 6)
    for region in (None, [p for p in s.points if want[p] == 1]):
        dense_region = mask if region is None else want == 1
        assert s.stats(region) == rr.stats(dense, dense_region)
    # the mesh, index for index, without and with relaxation
    for relax in (0, 3):
        V, T, info = s.mesh(relax)
        wV, wT, winfo = mr.mesh_region(mask, relax)
        assert info == winfo and np.array_equal(V, wV) and np.array_equal(T, wT), relax
    V0 = mr.mesh_region(mask, 0)[0]
    assert ((V0 % 256) != 0).all()                                                      # an unrelaxed vertex lies strictly inside its cell
    for name, fn, full in (("dilate 2", lambda m: mo.dilate(m > 0, 6, 2), mo.dilate(mask, 6, 2)),
                           ("erode 1", lambda m: mo.erode(m > 0, 26, 1), mo.erode(mask, 26, 1)),
                           ("to unset", lambda m: np.where(m > 0, dr.distance_map(m > 0, (1, 1, 1), dr.TO_UNSET), 0),
                            np.where(mask, dr.distance_map(mask, (1, 1, 1), dr.TO_UNSET), 0))):
        got = s.apply(4, fn)
        assert sorted(got) == [tuple(p) for p in np.argwhere(full).tolist()], name
        assert all(int(full[p]) == v for p, v in got.items()), name
