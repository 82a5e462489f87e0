"""Shapes, threshold mirrors and input builders of the scale tests (tests/test_scale_cpu.py, tests/test_scale_gpu.py): the smallest
volumes at which the launch code of the volume operations takes a second trip of a stride loop, splits a grid over a second dimension,
adds a scan level or passes 2^32 lanes, and the two large volumes whose byte offsets pass 2^31 and 2^32.  Nothing here touches a device.
Shapes are (nz, ny, nx)."""
import re
from pathlib import Path

import numpy as np

from sunvolumerender_amd import abi, host
from tests import distance_ref as dr
from tests import filter_ref as fr
from tests import label_ref as lr
from tests import region_ref as rr

CSRC = Path(__file__).resolve().parents[1] / "sunvolumerender_amd" / "csrc"

# ---------------------------------------------------------------------------------------------- mirrors of the launch constants
REGION_SPAN_BLOCKS = 2048                                # span_blocks of svr_region.hip: the cap of the classify / stats / apply grids
REGION_THREADS = 256                                     # THREADS of svr_region.hip: 4 waves, each walks spans of 64 lanes
REGION_WAVES = REGION_THREADS // 64
SMOOTH_ROWS = 8                                          # SVR_SMOOTH_ROWS of svr_filter.hip: the rows one block of a smoothing pass walks
RESAMPLE_ROWS = 4                                        # ROWS of svr_resample.hip: the output rows one block walks
GRID_Y_MAX = 65535                                       # the cap of gridDim.y in launch_smooth and row_grid
DISTANCE_MAX_BLOCKS = 2048                               # the cap of svr_region_distance_max's grid
BBOX_BLOCKS = 256                                        # BBOX_BLOCKS of svr_mesh.hip
LABEL_SCAN_BLOCK = abi.LABEL_SCAN_BLOCK                  # SVR_LABEL_SCAN_BLOCK of svr_label.hip
MASK_THREADS = 256                                       # MASK_THREADS of svr_mask.hpp

# name -> (file under csrc, a pattern whose group(s) hold the value in that file)
SOURCES = {
    "REGION_SPAN_BLOCKS": ("svr_region.hip", r"int span_blocks\(.*?want < (\d+)ull \? want : (\d+)ull"),
    "REGION_THREADS": ("svr_region.hip", r"constexpr int THREADS = (\d+);"),
    "SMOOTH_ROWS": ("svr_filter.hip", r"#define\s+SVR_SMOOTH_ROWS\s+(\d+)"),
    "RESAMPLE_ROWS": ("svr_resample.hip", r"constexpr uint32_t ROWS = (\d+);"),
    "GRID_Y_MAX filter": ("svr_filter.hip", r"gy = groups < (\d+)u \? groups : (\d+)u"),
    "GRID_Y_MAX resample": ("svr_resample.hip", r"gy = groups < (\d+)u \? groups : (\d+)u"),
    "DISTANCE_MAX_BLOCKS": ("svr_distance.hip", r"blocks = std::min<size_t>\(\(words \* 32 \+ THREADS - 1\) / THREADS, (\d+)\)"),
    "BBOX_BLOCKS": ("svr_mesh.hip", r"constexpr uint32_t BBOX_BLOCKS = (\d+);"),
    "LABEL_SCAN_BLOCK": ("svr_label.hip", r"#define\s+SVR_LABEL_SCAN_BLOCK\s+(\d+)"),
    "MASK_THREADS": ("svr_mask.hpp", r"constexpr int MASK_THREADS = (\d+);"),
}
MIRRORS = {"REGION_SPAN_BLOCKS": REGION_SPAN_BLOCKS, "REGION_THREADS": REGION_THREADS, "SMOOTH_ROWS": SMOOTH_ROWS, "RESAMPLE_ROWS": RESAMPLE_ROWS,
           "GRID_Y_MAX filter": GRID_Y_MAX, "GRID_Y_MAX resample": GRID_Y_MAX, "DISTANCE_MAX_BLOCKS": DISTANCE_MAX_BLOCKS, "BBOX_BLOCKS": BBOX_BLOCKS,
           "LABEL_SCAN_BLOCK": LABEL_SCAN_BLOCK, "MASK_THREADS": MASK_THREADS}


def source_values(name):
    """Every value the pattern of `name` captures in its source file (none if the text is gone)."""
    path, pattern = SOURCES[name]
    m = re.search(pattern, (CSRC / path).read_text(), re.S)
    return [int(g) for g in m.groups()] if m else []


# ---------------------------------------------------------------------------------------------- the quantities the thresholds are about
def voxels(shape):
    return int(shape[0]) * int(shape[1]) * int(shape[2])


def region_tasks(shape, vector):
    """The wave tasks of k_region_classify / _stats / _apply: rows times spans of 64 lanes of `vector` voxels."""
    nz, ny, nx = shape
    return nz * ny * ((nx + 64 * vector - 1) // (64 * vector))


REGION_TRIP = REGION_SPAN_BLOCKS * REGION_WAVES          # tasks of one trip of the capped grid


def row_grid(rows, rows_per_block):
    """(groups, gridDim.y, gridDim.z) of launch_smooth (svr_filter.hip) and row_grid (svr_resample.hip)."""
    groups = (rows + rows_per_block - 1) // rows_per_block
    gy = min(groups, GRID_Y_MAX)
    return groups, gy, (groups + gy - 1) // gy


def mask_words(shape):
    return host.region_mask_words(shape)


def lanes(shape):
    """The threads of a one-lane-per-voxel kernel: 32 per mask word."""
    return 32 * mask_words(shape)


DISTANCE_MAX_TRIP = DISTANCE_MAX_BLOCKS * MASK_THREADS   # lanes of one trip of k_dist_max
BBOX_TRIP = BBOX_BLOCKS * MASK_THREADS                   # vertices of one trip of k_mesh_bbox

# ---------------------------------------------------------------------------------------------- mid tier: shapes
REGION_SHAPES = {8: (96, 96, 40), 1: (96, 96, 37)}       # vector width of the path -> shape: 9 216 tasks each
FILTER_SHAPE = (725, 724, 3)                             # 524 900 rows, 65 613 groups of 8: gridDim.z = 2
RESAMPLE_OUT = (513, 512, 3)                             # 262 656 output rows, 65 664 groups of 4: gridDim.z = 2
DISTANCE_SHAPE = (64, 64, 160)                           # 20 480 mask words, 655 360 lanes
MESH_SHAPE = (48, 48, 48)
LABEL_SHAPE = (4097, 4096, 1)                            # 16 781 312 mask words: four scan levels
NARROW_SHAPE = (8192, 16384, 1)                          # 2^27 mask words, 2^32 lanes


# ---------------------------------------------------------------------------------------------- mid tier: inputs
def region_case(vector):
    """(vox, seeds (x, y, z), region, stats) of the noise volume of the `vector` path; the seed lies in the cluster that percolates."""
    shape = REGION_SHAPES[vector]
    vox = rr.noise_volume(shape, seed=70 + vector)
    seeds = rr.spread_seeds(vox)[1:2]
    region, stats = rr.reference("scale", vox, seeds, rr.NOISE_LO, rr.NOISE_HI, 6)
    return vox, seeds, region, stats


def filter_volume():
    return rr.cached(("scale", "filter volume"), lambda: fr.random_volume(FILTER_SHAPE, 71))


RESAMPLE_GRIDS = {                                       # name -> the steps of x, y, z: none of them the copy
    "nearest": (98304, 43691, 131072),
    "linear": (43691, 98304, 32768),
    "area": (131072, 65537, 98304),
}
RESAMPLE_CROP_OFFSET = (2, 5, 3)                         # x, y, z of the crop-only case
RESAMPLE_CROP_SOURCE = (518, 519, 7)


def resample_grid(name):
    """The grid of a named case onto RESAMPLE_OUT, ((origin, step, count) of x, of y, of z), with fractional origins."""
    if name == "crop":
        return tuple((o << 16, 65536, n) for o, n in zip(RESAMPLE_CROP_OFFSET, RESAMPLE_OUT[::-1]))
    return tuple((origin, step, n) for origin, step, n in zip((-20000, 12345, 7), RESAMPLE_GRIDS[name], RESAMPLE_OUT[::-1]))


def resample_source_shape(name):
    """The smallest source that holds every sample of the grid (the last ones may still clamp at the far face)."""
    if name == "crop":
        return RESAMPLE_CROP_SOURCE
    return tuple(max(1, (origin + step * count) >> 16) for origin, step, count in resample_grid(name))[::-1]


def garbage_padded(mask, seed):
    """The words of a bool mask with random bits in the padding of every row's last word."""
    nz, ny, nx = mask.shape
    words = rr.pack(mask).reshape(nz, ny, -1).copy()
    if nx % 32:
        junk = np.random.default_rng(seed).integers(0, 1 << 32, size=(nz, ny), dtype=np.uint64).astype(np.uint32)
        words[:, :, -1] |= junk & np.uint32((0xFFFFFFFF << (nx % 32)) & 0xFFFFFFFF)
    return np.ascontiguousarray(words.reshape(-1))


def distance_lane(zyx, shape=DISTANCE_SHAPE):
    """The lane of voxel (z, y, x) in a one-lane-per-voxel kernel: 32 per mask word."""
    nz, ny, nx = shape
    z, y, x = zyx
    return ((z * ny + y) * ((nx + 31) // 32) + (x >> 5)) * 32 + (x & 31)


DISTANCE_EARLY = (10, 20, 30)                            # a voxel of the first trip of k_dist_max
DISTANCE_LATE = (55, 33, 140)                            # one that only the second trip reaches
DISTANCE_PEAK = 5000                                     # above every value of the noise map


def distance_map_noise():
    """A uint32 map of values below DISTANCE_PEAK with SVR_DIST_NONE entries sprinkled in (svr_region_distance_max takes any map)."""
    rng = np.random.default_rng(72)
    m = rng.integers(0, DISTANCE_PEAK, size=DISTANCE_SHAPE, dtype=np.uint32)
    m[rng.random(DISTANCE_SHAPE) < 0.05] = dr.NONE
    return m


def mesh_mask():
    return np.random.default_rng(73).random(MESH_SHAPE) < 0.5


def label_random(shape=LABEL_SHAPE):
    return np.random.default_rng(74).random(shape) < 0.45


def label_checker(shape=LABEL_SHAPE):
    """Every other voxel of a one-voxel-wide volume: under 6-connectivity each set voxel is a component."""
    nz, ny, nx = shape
    assert nx == 1
    return ((np.arange(nz)[:, None] + np.arange(ny)[None, :]) % 2 == 0).reshape(shape)


def label_checker_count(shape=LABEL_SHAPE):
    return (shape[0] * shape[1] + 1) // 2


def scipy_label(mask, connectivity):
    """(labels uint32, K) by scipy.ndimage.label; tests/test_label_cpu.py shows that it numbers components as tests/label_ref.py does:
    by their first voxel in scan order."""
    from scipy import ndimage

    structure = np.zeros((3, 3, 3), dtype=bool)
    for o in rr.offsets(connectivity):
        structure[o[0] + 1, o[1] + 1, o[2] + 1] = True
    structure[1, 1, 1] = True
    out = np.empty(mask.shape, dtype=np.int32)
    k = ndimage.label(mask, structure=structure, output=out)
    return out.view(np.uint32), int(k)


def fast_table(labels, count):
    """tests/label_ref.py's table (voxels, first, bbox_min, bbox_max; sum 0) by one stable sort instead of ufunc.at: for millions of labels."""
    flat = labels.reshape(-1)
    on = np.flatnonzero(flat)
    lab = flat[on].astype(np.int64) - 1
    order = np.argsort(lab, kind="stable")
    sizes = np.bincount(lab, minlength=count)
    assert (sizes > 0).all()
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    zyx = np.unravel_index(on[order], labels.shape)
    t = {"voxels": sizes.astype(np.uint32), "first": on[order][starts].astype(np.uint32), "sum": np.zeros(count, dtype=np.uint64),
         "bbox_min": np.empty((count, 3), dtype=np.int32), "bbox_max": np.empty((count, 3), dtype=np.int32)}
    for a, c in enumerate(zyx[::-1]):                    # x, y, z
        t["bbox_min"][:, a] = np.minimum.reduceat(c, starts)
        t["bbox_max"][:, a] = np.maximum.reduceat(c, starts)
    return t


def fast_kept(sizes, min_voxels, largest_k):
    """tests/label_ref.py's kept_labels as a keep array indexed by label, by one lexsort: larger first, ties to the lower label."""
    sizes = np.asarray(sizes, dtype=np.int64)
    order = np.lexsort((np.arange(len(sizes)), -sizes))
    order = order[(sizes[order] >= min_voxels) & (sizes[order] > 0)]
    if largest_k:
        order = order[:largest_k]
    keep = np.zeros(len(sizes) + 1, dtype=np.uint8)
    keep[order + 1] = 1
    return keep


# ---------------------------------------------------------------------------------------------- sparse contents of very large volumes
class Sparse:
    """A volume that is background everywhere but at a few voxels: {(z, y, x): value}.  Expected results come from the small references
    run on CUT-OUTS: the boxes of the clusters of voxels, with a margin, clipped to the volume -- a cut-out's face is the volume's face
    exactly where the two coincide, which is what the border rules of the operations need."""

    def __init__(self, shape, points):
        self.shape = tuple(int(n) for n in shape)
        self.points = {tuple(int(c) for c in p): int(v) for p, v in points.items()}
        for z, y, x in self.points:
            assert 0 <= z < shape[0] and 0 <= y < shape[1] and 0 <= x < shape[2], (z, y, x)

    def index(self, zyx):
        nz, ny, nx = self.shape
        return (zyx[0] * ny + zyx[1]) * nx + zyx[2]

    def indices(self):
        """(sorted linear indices int64, their values)"""
        items = sorted((self.index(p), v) for p, v in self.points.items())
        return np.array([i for i, _ in items], dtype=np.int64), np.array([v for _, v in items], dtype=np.int64)

    def x_runs(self):
        """[(linear index of the first voxel, [values])]: the maximal runs along x, for uploads."""
        runs = []
        for i, v in zip(*self.indices()):
            if runs and runs[-1][0] + len(runs[-1][1]) == i and i % self.shape[2] != 0:
                runs[-1][1].append(int(v))
            else:
                runs.append((int(i), [int(v)]))
        return runs

    def cutouts(self, margin):
        """[(z0, y0, x0), (z1, y1, x1)] half-open boxes: the points' boxes grown by `margin`, merged while any two touch or overlap."""
        boxes = [[[max(0, c - margin) for c in p], [min(n, c + margin + 1) for c, n in zip(p, self.shape)]] for p in self.points]
        merged = True
        while merged:
            merged = False
            out = []
            for b in boxes:
                for o in out:
                    if all(b[0][a] <= o[1][a] and o[0][a] <= b[1][a] for a in range(3)):
                        o[0] = [min(p, q) for p, q in zip(o[0], b[0])]
                        o[1] = [max(p, q) for p, q in zip(o[1], b[1])]
                        merged = True
                        break
                else:
                    out.append(b)
            boxes = out
        return sorted((tuple(b[0]), tuple(b[1])) for b in boxes)

    def cut(self, box, dtype=np.uint16, background=0):
        """The dense contents of a cut-out."""
        (z0, y0, x0), (z1, y1, x1) = box
        a = np.full((z1 - z0, y1 - y0, x1 - x0), background, dtype=dtype)
        for (z, y, x), v in self.points.items():
            if z0 <= z < z1 and y0 <= y < y1 and x0 <= x < x1:
                a[z - z0, y - y0, x - x0] = v
        return a

    def apply(self, margin, fn, dtype=np.uint16, background=0):
        """{(z, y, x): value} of the non-zero voxels of fn(cut-out) over all cut-outs: the sparse result of a local operation whose
        result on the background alone is 0 and whose reach is below `margin`.  Asserts that nothing arrives at a cut-out's inner faces."""
        out = {}
        for box in self.cutouts(margin):
            res = np.asarray(fn(self.cut(box, dtype, background)))
            (z0, y0, x0), (z1, y1, x1) = box
            for a, (lo, hi, n) in enumerate(((z0, z1, self.shape[0]), (y0, y1, self.shape[1]), (x0, x1, self.shape[2]))):
                if lo > 0:
                    assert not np.take(res, 0, axis=a).any(), "the margin is too small for the operation"
                if hi < n:
                    assert not np.take(res, hi - lo - 1, axis=a).any(), "the margin is too small for the operation"
            for z, y, x in np.argwhere(res):
                out[(int(z) + z0, int(y) + y0, int(x) + x0)] = int(res[z, y, x])
        return out

    def stats(self, region=None):
        """tests/region_ref.py's stats of the region `region` (points; None = all) from the definitions, in Python integers."""
        pts = self.points if region is None else {p: self.points[p] for p in region}
        nz, ny, nx = self.shape
        v = list(pts.values())
        s = {"voxels": len(pts), "sum": sum(v), "sum_sq": sum(t * t for t in v), "sum_x": sum(p[2] for p in pts), "sum_y": sum(p[1] for p in pts),
             "sum_z": sum(p[0] for p in pts)}
        for name, a in (("faces_x", 2), ("faces_y", 1), ("faces_z", 0)):
            s[name] = sum(1 for p in pts for sgn in (1, -1) if tuple(c + sgn * (i == a) for i, c in enumerate(p)) not in pts)
        if pts:
            s["vmin"], s["vmax"] = min(v), max(v)
            s["bbox_min"] = [min(p[a] for p in pts) for a in (2, 1, 0)]
            s["bbox_max"] = [max(p[a] for p in pts) for a in (2, 1, 0)]
        else:
            s["vmin"], s["vmax"], s["bbox_min"], s["bbox_max"] = 65535, 0, [nx, ny, nz], [-1, -1, -1]
        s["status"] = rr.OK if pts else rr.EMPTY
        return s

    def mesh(self, relax=0):
        """tests/mesh_ref.py's mesh of the mask of the points, from the mesh of the squeezed mask: a cell of the surface net sees its
        eight corners only and no active cell spans a squeezed gap, so vertices, their order and the triangles are those of the large
        volume once every vertex is moved back to its cell there."""
        from tests import mesh_ref

        small, _ = self.squeeze()
        coords = self.squeezed_coords()
        V0, T, info = mesh_ref.mesh_region(small, 0)
        V = V0 if relax == 0 else mesh_ref.mesh_region(small, relax)[0]
        cell = V0 // 256                                 # (an unrelaxed vertex lies strictly inside its cell: see the CPU test)
        out = np.empty_like(V)
        for a in range(3):                               # x, y, z; cell i spans voxels i - 1 and i
            c = np.array(coords[2 - a] + [coords[2 - a][-1] + 1], dtype=np.int64)
            out[:, a] = V[:, a] - 256 * cell[:, a] + 256 * c[cell[:, a]]
        info = dict(info, bbox_min=out.min(axis=0).tolist(), bbox_max=out.max(axis=0).tolist())
        return out.astype(np.int32), T, info

    def squeezed_coords(self):
        """Per axis (z, y, x) the coordinates that squeeze() keeps, ascending: the used ones and their neighbours."""
        return [sorted({c for p in self.points for c in (p[a] - 1, p[a], p[a] + 1) if 0 <= c < self.shape[a]}) for a in range(3)]

    def squeeze(self):
        """(dense bool array, {point: its place}) with every run of unused coordinates shrunk to its two end planes (or its one): adjacency
        between the points, the faces they touch and their scan order are those of the large volume, so components and their numbering are."""
        keep, place = [], []
        for a in range(3):
            used = sorted({p[a] for p in self.points})
            coords = sorted({c for u in used for c in (u - 1, u, u + 1) if 0 <= c < self.shape[a]})
            # (u - 1 and u + 1 stay as the empty planes; further unused ones between two kept coordinates only shrink)
            keep.append(coords)
            place.append({c: i for i, c in enumerate(coords)})
        small = np.zeros(tuple(len(k) for k in keep), dtype=bool)
        where = {}
        for p in self.points:
            q = tuple(place[a][p[a]] for a in range(3))
            small[q] = True
            where[p] = q
        # two kept coordinates that are not neighbours in the volume must not become neighbours: there is a kept empty plane between them
        for a in range(3):
            used = sorted({p[a] for p in self.points})
            for u, v in zip(used, used[1:]):
                assert v - u == 1 or place[a][v] - place[a][u] >= 2
        return small, where

    def labels(self, connectivity):
        """({point: label}, K) of the mask of the points."""
        small, where = self.squeeze()
        lab, k = lr.label(small, connectivity)
        return {p: int(lab[q]) for p, q in where.items()}, k

    def table(self, labelling, count, values=None):
        """tests/label_ref.py's table of a sparse labelling {point: label}; sum from {point: value} if given."""
        t = {"voxels": np.zeros(count, dtype=np.uint32), "first": np.full(count, 0xFFFFFFFF, dtype=np.uint32), "sum": np.zeros(count, dtype=np.uint64),
             "bbox_min": np.full((count, 3), np.iinfo(np.int32).max, dtype=np.int32), "bbox_max": np.full((count, 3), -1, dtype=np.int32)}
        for p, lab in labelling.items():
            i = lab - 1
            t["voxels"][i] += 1
            t["first"][i] = min(int(t["first"][i]), self.index(p))
            for a, c in enumerate(p[::-1]):
                t["bbox_min"][i, a] = min(int(t["bbox_min"][i, a]), c)
                t["bbox_max"][i, a] = max(int(t["bbox_max"][i, a]), c)
            if values is not None:
                t["sum"][i] += values[p]
        return t


def sparse_words(shape, points):
    """(word indices int64 ascending, words uint32) of the mask whose set voxels are `points`: every other word is 0."""
    nz, ny, nx = shape
    wx = (nx + 31) // 32
    words = {}
    for z, y, x in points:
        w = (z * ny + y) * wx + (x >> 5)
        words[w] = words.get(w, 0) | (1 << (x & 31))
    idx = np.array(sorted(words), dtype=np.int64)
    return idx, np.array([words[int(i)] for i in idx], dtype=np.uint32)


def narrow_points(shape=NARROW_SHAPE):
    """{(z, y, 0): value} of the narrow volume: short runs along y and along z at the first row, the last row and on both sides of rows
    2^26 and 2^27 - 1 (row = z * ny + y = the mask word = the voxel), every value distinct and in the window NARROW_WINDOW."""
    nz, ny, nx = shape
    assert nx == 1 and ny * 4096 == 1 << 26 and nz * ny == 1 << 27
    cells = []
    cells += [(0, y) for y in range(5)] + [(z, 0) for z in range(1, 3)]                           # the first row on: an L
    cells += [(4095, y) for y in range(ny - 4, ny)]                                               # rows 2^26 - 4 .. 2^26 - 1
    cells += [(4096, y) for y in range(4)] + [(z, 0) for z in (4094, 4095, 4097)]                 # row 2^26 on, and a run along z through it
    cells += [(z, 777) for z in range(4094, 4099)]                                                # a run along z on its own
    cells += [(nz - 1, y) for y in range(ny - 4, ny)] + [(z, ny - 1) for z in range(nz - 3, nz - 1)]   # up to row 2^27 - 1: the last
    cells += [(nz - 1, 0), (0, ny - 1)]                                                           # the other two corners, single voxels
    assert len(set(cells)) == len(cells)
    return {(z, y, 0): 1000 + i for i, (z, y) in enumerate(cells)}


NARROW_WINDOW = (1000, 1999)

# ---------------------------------------------------------------------------------------------- large tier
L1 = (512, 1024, 1024)                                   # 2^29 voxels: uint32 maps of 2 GiB, geodesic keys of 4 GiB
L2 = (2048, 1024, 1024)                                  # 2^31 voxels, the most a call admits: u16 of 4 GiB, uint32 maps of 8 GiB
BEACON = 5                                               # the edge of a beacon block
BEACON_WINDOW = (2000, 9999)


def plane_crossings(shape):
    """The voxel indices 2^28, 2^29, 2^30 and 3 * 2^29 that lie inside the volume."""
    return [i for i in (1 << 28, 1 << 29, 1 << 30, 3 << 29) if i < voxels(shape)]


ROD = 7                                                  # the voxels of a rod: the gap between a beacon and its companion


def beacon_origins(shape):
    """(z, y, x) of the low corner of every beacon: the eight corners of the volume (the far one ends at the last voxel); one block
    straddling each plane where the voxel index passes 2^28, 2^29, 2^30 and 3 * 2^29 (a z plane, in these shapes), off the faces and
    across a mask word in x; then the COMPANIONS of the origin corner, the far corner and every plane beacon, ROD voxels away along x."""
    nz, ny, nx = shape
    b = BEACON
    at = [(z, y, x) for z in (0, nz - b) for y in (0, ny - b) for x in (0, nx - b)]
    for i in plane_crossings(shape):
        assert i % (ny * nx) == 0
        z = i // (ny * nx)
        at.append((z - 2, 300 + (z % 7) * 40, 512 + (z % 5) * 32 - 2))
    return at + [(z, y, x + b + ROD if x + 2 * b + ROD <= nx else x - b - ROD) for z, y, x in [at[0], at[7]] + at[8:]]


def beacon_rods(shape):
    """[[(z, y, x), ...]]: the one-voxel rods along x through the centres of a beacon and its companion."""
    at = beacon_origins(shape)
    pairs = len(at) - 8 - len(plane_crossings(shape))
    rods = []
    for (z, y, x), (_, _, cx) in zip([at[0], at[7]] + at[8:8 + len(plane_crossings(shape))], at[-pairs:]):
        lo = min(x, cx) + BEACON
        rods.append([(z + 2, y + 2, lo + i) for i in range(ROD)])
    return rods


def beacon_points(shape):
    """{(z, y, x): value}: 5 x 5 x 5 blocks and the rods, every value distinct and inside BEACON_WINDOW."""
    pts, v = {}, BEACON_WINDOW[0]
    for z0, y0, x0 in beacon_origins(shape):
        for dz in range(BEACON):
            for dy in range(BEACON):
                for dx in range(BEACON):
                    pts[(z0 + dz, y0 + dy, x0 + dx)] = v
                    v += 1
    for rod in beacon_rods(shape):
        for p in rod:
            assert p not in pts
            pts[p] = v
            v += 1
    assert max(pts.values()) <= BEACON_WINDOW[1]
    return pts


def beacon_components(shape):
    return len(beacon_origins(shape)) - len(beacon_rods(shape))


HOLLOW_BEACON = 8                                        # of beacon_origins: the first plane beacon loses its centre in the morph test


def hollow_centre(shape):
    z, y, x = beacon_origins(shape)[HOLLOW_BEACON]
    return (z + 2, y + 2, x + 2)


def rod_points(shape=L1):
    """The rod domain of the geodesic and grow-from-seeds tests: the last column of the volume along z from z = 251 on, through the
    plane where the voxel index passes 2^28 (z = 256) up to the last voxel, 2^29 - 1; with the u16 value of each voxel."""
    nz, ny, nx = shape
    return {(z, ny - 1, nx - 1): (z * 37) % 1000 for z in range(251, nz)}
