"""The numpy reference of the surface-nets meshes (svr_mesh_isosurface / svr_mesh_region; the definitions are restated in
include/svr_abi.h and DESIGN.md 8o): vectorised, integers only, every array in the order the contract fixes, so the GPU's output is
compared index for index.  Arrays are [nz][ny][nx]; a vertex is (x, y, z) in units of 1/256 voxel on the padded grid, u = 256 (x + 1)."""
import numpy as np

NONE = -1
STATUS_OK, STATUS_EMPTY = 0, 1
AXES = ((0, 1, 2), (1, 2, 0), (2, 0, 1))                 # (a, b, c) cyclic
FACES = ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1))  # (axis, side): -x, +x, -y, +y, -z, +z


def mask_field(mask):
    """The field of a region mask: 2 inside, 0 outside, to be taken at level 1."""
    return np.where(np.asarray(mask, dtype=bool), 2, 0).astype(np.uint16)


def _padded(vox):
    vox = np.asarray(vox)
    nz, ny, nx = vox.shape
    v = np.zeros((nz + 3, ny + 3, nx + 3), dtype=np.int64)   # one virtual layer before, two after: every corner of every padded point exists
    v[1:nz + 1, 1:ny + 1, 1:nx + 1] = vox
    return v


def _corner(a, off, shape):
    """the array of corner `off` = (ox, oy, oz) of every cell"""
    cz, cy, cx = shape
    return a[off[2]:off[2] + cz, off[1]:off[1] + cy, off[0]:off[0] + cx]


def mesh(vox, level, relax=0):
    """(vertices int32 [nv, 3], triangles uint32 [nt, 3], info) of the field `vox` at `level`."""
    vox = np.asarray(vox)
    nz, ny, nx = vox.shape
    assert 1 <= level <= 65535 and 0 <= relax <= 64
    v = _padded(vox)
    ins = v >= level
    cells = (nz + 1, ny + 1, nx + 1)
    offs = [(o & 1, (o >> 1) & 1, (o >> 2) & 1) for o in range(8)]
    cin = [_corner(ins, o, cells) for o in offs]
    cval = [_corner(v, o, cells) for o in offs]
    count = sum(c.astype(np.int64) for c in cin)
    active = (count > 0) & (count < 8)
    nv = int(active.sum())
    info = {"vertices": nv, "quads": 0, "triangles": 0, "bbox_min": [256 * (nx + 2), 256 * (ny + 2), 256 * (nz + 2)], "bbox_max": [-1, -1, -1],
            "status": STATUS_EMPTY}
    if nv == 0:
        return np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), info
    vid = np.full((nz + 2, ny + 2, nx + 2), NONE, dtype=np.int64)
    vid[:nz + 1, :ny + 1, :nx + 1][active] = np.arange(nv)                      # C order = ascending linear cell index

    # ---- vertices: the rounded mean of the crossing points of the cell's 12 edges
    S = [np.zeros(cells, np.int64) for _ in range(3)]
    m = np.zeros(cells, np.int64)
    for a, b, c in AXES:
        for ob in (0, 1):
            for oc in (0, 1):
                lo = (ob << b) | (oc << c)
                hi = lo | (1 << a)
                cross = cin[lo] != cin[hi]
                vi = np.where(cin[lo], cval[lo], cval[hi])
                vo = np.where(cin[lo], cval[hi], cval[lo])
                den = np.where(cross, vi - vo, 1)
                q = (256 * (level - vo)) // den
                t = np.where(cin[lo], 256 - q, q)
                S[a] += np.where(cross, t, 0)
                S[b] += np.where(cross, 256 * ob, 0)
                S[c] += np.where(cross, 256 * oc, 0)
                m += cross
    kk, jj, ii = np.nonzero(active)
    base = [256 * ii, 256 * jj, 256 * kk]
    ma = m[active]
    assert ma.min() >= 3 and ma.max() <= 12
    V = np.stack([base[a] + (2 * S[a][active] + ma) // (2 * ma) for a in range(3)], axis=1)

    # ---- quads: one per crossing edge s -> s + e_a, ordered by 3 * index(s) + a
    pin = ins[:nz + 2, :ny + 2, :nx + 2]
    keys, quads = [], []
    for a, b, c in AXES:
        nxt = _corner(ins, tuple(int(t == a) for t in range(3)), (nz + 2, ny + 2, nx + 2))
        z, y, x = np.nonzero(pin != nxt)
        p = [x, y, z]
        s_in = pin[z, y, x]

        def cell(db, dc):
            t = [p[0].copy(), p[1].copy(), p[2].copy()]
            t[b] += db
            t[c] += dc
            assert all(t[i].min(initial=0) >= 0 for i in range(3))
            return vid[t[2], t[1], t[0]]
        c00, c10, c11, c01 = cell(-1, -1), cell(0, -1), cell(0, 0), cell(-1, 0)
        q = np.where(s_in[:, None], np.stack([c00, c10, c11, c01], axis=1), np.stack([c00, c01, c11, c10], axis=1))
        keys.append(3 * ((z * (ny + 2) + y) * (nx + 2) + x) + a)
        quads.append(q)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    quads = quads[np.argsort(keys, kind="stable")]
    assert quads.min() >= 0
    T = np.empty((2 * len(quads), 3), np.int64)
    T[0::2] = quads[:, [0, 1, 2]]
    T[1::2] = quads[:, [0, 2, 3]]

    # ---- relaxation: Jacobi steps towards the mean of the linked neighbours, clamped to the cell
    if relax:
        bits = sum(cin[o].astype(np.int64) << o for o in range(8))[active]
        nb = np.full((nv, 6), NONE, dtype=np.int64)
        for f, (a, side) in enumerate(FACES):
            sel = sum(1 << o for o in range(8) if ((o >> a) & 1) == side)
            fb = bits & sel
            mixed = (fb != 0) & (fb != sel)
            t = [ii.copy(), jj.copy(), kk.copy()]
            t[a] += 1 if side else -1
            ok = np.nonzero(mixed)[0]
            assert all(t[i][ok].min(initial=0) >= 0 for i in range(3))
            nb[ok, f] = vid[t[2][ok], t[1][ok], t[0][ok]]
            assert (nb[ok, f] >= 0).all()
        have = nb >= 0
        links = have.sum(axis=1)
        assert links.min() >= 3
        lo = np.stack(base, axis=1)
        for _ in range(relax):
            total = np.where(have[:, :, None], V[np.where(have, nb, 0)], 0).sum(axis=1)
            V = np.clip((2 * total + links[:, None]) // (2 * links[:, None]), lo, lo + 256)

    info.update(vertices=nv, quads=len(quads), triangles=len(T), bbox_min=V.min(axis=0).tolist(), bbox_max=V.max(axis=0).tolist(), status=STATUS_OK)
    return V.astype(np.int32), T.astype(np.uint32), info


def mesh_region(mask, relax=0):
    return mesh(mask_field(mask), 1, relax)


def _cells(vox, level):
    """(i, j, k) [nv, 3] of the active cells, in vertex order"""
    nz, ny, nx = np.asarray(vox).shape
    ins = _padded(vox) >= level
    cells = (nz + 1, ny + 1, nx + 1)
    count = sum(_corner(ins, (o & 1, (o >> 1) & 1, (o >> 2) & 1), cells).astype(np.int64) for o in range(8))
    kk, jj, ii = np.nonzero((count > 0) & (count < 8))
    return np.stack([ii, jj, kk], axis=1)


def closed_and_oriented(T):
    """every directed edge of the triangles is met by its reverse, as multisets: the mesh is closed and consistently oriented"""
    T = np.asarray(T, dtype=np.int64)
    if len(T) == 0:
        return True
    n = int(T.max()) + 1
    a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]])
    b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]])
    return bool(np.array_equal(np.sort(a * n + b), np.sort(b * n + a)))


def directed_edge_counts(T):
    T = np.asarray(T, dtype=np.int64)
    n = int(T.max()) + 1
    a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]])
    b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]])
    return np.unique(a * n + b, return_counts=True)[1]


def euler(V, T):
    T = np.asarray(T, dtype=np.int64)
    n = len(V)
    a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]])
    b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]])
    edges = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    return n - len(edges) + len(T)


def volume6(V, T):
    """sum of a . (b x c) over the triangles in wrap-around int64: 6 * 256^3 * the enclosed volume in voxels"""
    V = np.asarray(V, dtype=np.int64)
    T = np.asarray(T, dtype=np.int64)
    if len(T) == 0:
        return 0
    a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    with np.errstate(over="ignore"):
        return int(np.sum(np.sum(a * np.cross(b, c), axis=1), dtype=np.int64))


def area(V, T, scale):
    """sum of 1/2 |((b - a) o s) x ((c - a) o s)| in float64"""
    V = np.asarray(V, dtype=np.float64) * np.asarray(scale, dtype=np.float64)
    T = np.asarray(T, dtype=np.int64)
    if len(T) == 0:
        return 0.0
    a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    n = np.cross(b - a, c - a)
    return float(0.5 * np.sqrt((n * n).sum(axis=1)).sum())


def positions_mm(V, spacing):
    return ((np.asarray(V, dtype=np.float64) / 256.0 - 0.5) * np.asarray(spacing, dtype=np.float64)).astype(np.float32)


def ball(n=24, radius=9.0):
    """a ramped ball: 40000 at the centre, falling linearly to 0 at 2 * radius; level 20000 is the sphere of `radius`"""
    z, y, x = np.mgrid[:n, :n, :n].astype(np.float64) - (n - 1) / 2.0
    r = np.sqrt(x * x + y * y + z * z)
    return np.clip(40000.0 * (1.0 - r / (2.0 * radius)), 0, 65535).astype(np.uint16)


def torus(n=24, R=7.0, r=3.0):
    """a ramped torus around the z axis: level 20000 is the torus of radii R, r"""
    z, y, x = np.mgrid[:n, :n, :n].astype(np.float64) - (n - 1) / 2.0
    d = np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z)
    return np.clip(40000.0 * (1.0 - d / (2.0 * r)), 0, 65535).astype(np.uint16)


def noise(shape, seed=5, hi=65536):
    return np.random.default_rng(seed).integers(0, hi, size=shape, dtype=np.int64).astype(np.uint16)
