"""The macro-grid rule (svr_macro_grid, plain host code) swept over shapes, and tests/accel_ref.py -- the numpy restatement of the
skipping tables that tests/test_accel_gpu.py compares the device's tables with -- anchored on the oracle's own sampler and checked
for non-vacuity.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding
from sunvolumerender_amd import abi, scenes
from tests import accel_ref as ar

f32 = np.float32
FLAT_SHAPES = [(512, 512, 1), (400, 330, 1), (1024, 1024, 2), (65538, 1, 1)]          # limited by the half-resolution grid


# ------------------------------------------------------------------------------------------------ the grid rule
def _parent_rule(nx, ny, nz, shift_min):
    """The rule before the half-resolution capacity was part of it: the smallest shift whose grid has at most 64^3 cells."""
    sh = shift_min
    while True:
        g = [((n - 1) >> sh) + 1 for n in (nx, ny, nz)]
        if g[0] * g[1] * g[2] <= 8192 * 32:
            return sh, g
        sh += 1


def _sweep_shapes():
    rs = np.random.RandomState(5)
    shapes = list(FLAT_SHAPES) + [(2048, 2048, 4), (300000, 1, 1), (1, 300000, 1), (1, 1, 300000), (1, 400, 330), (37, 21, 10), (40, 8, 8),
                                  (64, 64, 64), (48, 48, 48), (128, 128, 128), (512, 512, 512), (1024, 1024, 1024), (2048, 2048, 2048)]
    shapes += [(a, b, c) for a in (1, 2, 3) for b in (1, 2, 3, 700) for c in (1, 2, 3, 129, 4097)]
    for _ in range(3000):
        kind = rs.randint(4)
        if kind == 0:                                                      # box-like
            shapes.append(tuple(int(v) for v in rs.randint(1, 1400, 3)))
        elif kind == 1:                                                    # flat: one thin axis, anywhere
            s = [int(rs.randint(1, 3000)), int(rs.randint(1, 3000)), int(rs.randint(1, 5))]
            rs.shuffle(s)
            shapes.append(tuple(s))
        elif kind == 2:                                                    # a line
            s = [int(rs.randint(1, 400000)), int(rs.randint(1, 4)), int(rs.randint(1, 4))]
            rs.shuffle(s)
            shapes.append(tuple(s))
        else:                                                              # around the capacities: grids of about 64^3 / 32^3 cells
            e = rs.randint(0, 4)
            shapes.append(tuple(int(v) for v in (64 << e) + rs.randint(-2, 3, 3)))
    return shapes


def test_macro_grid_rule_sweep():
    """svr_macro_grid over a few thousand shapes x every SVR_OPT_MACRO_SHIFT_MIN: both capacities hold, the shift is the smallest that
    does, and wherever the rule without the half-resolution capacity already satisfied it the result is that rule's (every cubic and
    box-like shape: nothing of the committed fixtures or the benchmark moves)."""
    lib = abi.load()
    out = (C.c_int * 8)()
    moved = set()
    shapes = _sweep_shapes()
    assert len(shapes) > 3000
    for nx, ny, nz in shapes:
        for smin in range(7):
            sh = lib.svr_macro_grid(nx, ny, nz, smin, out)
            o = list(out)
            g, hg = o[1:4], o[4:7]
            what = f"{nx}x{ny}x{nz} shift_min {smin}: {o}"
            assert sh == o[0] >= smin, what
            assert g == [((n - 1) >> sh) + 1 for n in (nx, ny, nz)] and hg == [(c + 1) // 2 for c in g], what
            n, hn = g[0] * g[1] * g[2], hg[0] * hg[1] * hg[2]
            assert n <= ar.MASK_WORDS_MAX * 32 and hn <= ar.DIST_WORDS_MAX * 8 and o[7] == ar.ceil_div(hn, 8) <= ar.DIST_WORDS_MAX, what
            if sh > smin:                                                  # minimal: one less violates a capacity
                g1 = [((n_ - 1) >> (sh - 1)) + 1 for n_ in (nx, ny, nz)]
                h1 = [(c + 1) // 2 for c in g1]
                assert g1[0] * g1[1] * g1[2] > ar.MASK_WORDS_MAX * 32 or h1[0] * h1[1] * h1[2] > ar.DIST_WORDS_MAX * 8, what
            assert (sh, tuple(g), tuple(hg)) == ar.macro_grid(nx, ny, nz, smin), what
            psh, pg = _parent_rule(nx, ny, nz, smin)
            ph = [(c + 1) // 2 for c in pg]
            if ph[0] * ph[1] * ph[2] <= ar.DIST_WORDS_MAX * 8:
                assert (sh, g) == (psh, pg), what
            else:
                assert sh > psh, what
                moved.add((nx, ny, nz))
    for s in FLAT_SHAPES:
        assert s in moved, f"{s} must get a coarser grid than the 64^3 rule alone gives it"
        assert lib.svr_macro_grid(*s, 0, out) == _parent_rule(*s, 0)[0] + 1
    # not only thin shapes: a box whose grid has an ODD dimension rounds its half-resolution grid up -- 129 x 126 x 127 had a 65 x 63 x 64
    # grid (262 080 cells: fits) with 33 x 32 x 32 = 33 792 half-resolution cells (does not)
    assert lib.svr_macro_grid(129, 126, 127, 0, out) == 2 and _parent_rule(129, 126, 127, 0) == (1, [65, 63, 64])
    for n in (32, 48, 64, 128, 256, 512, 1024, 2048):                      # the cubes of the fixtures and the benchmark
        assert (n, n, n) not in moved and lib.svr_macro_grid(n, n, n, 0, out) == _parent_rule(n, n, n, 0)[0]
    assert lib.svr_macro_grid(0, 4, 4, 0, out) == -1 and lib.svr_macro_grid(4, 4, 4, -1, out) == -1 and lib.svr_macro_grid(4, 4, 4, 0, None) == -1


# ------------------------------------------------------------------------------------------------ pieces of the reference
@pytest.mark.parametrize("density_scale", [1.0, 37.5, -1.0, 0.3333333])
def test_lut_floor_against_rational_arithmetic(density_scale):
    """The float64 evaluation of the look-up coordinate's fma (accel_ref.lut_floor_of_raw, with the argument there) against exact
    rational arithmetic with one rounding to float32: every 5th raw value and every value around the places where the coordinate
    crosses an integer."""
    n = 1024
    table = ar.lut_floor_of_raw(density_scale, n)
    crossings = np.flatnonzero(np.diff(table) != 0)
    raws = set(range(0, 65536, 5)) | {0, 1, 2, 65534, 65535}
    for c in crossings[:: max(1, len(crossings) // 400)]:
        raws |= {int(c) - 1, int(c), int(c) + 1, int(c) + 2} & set(range(65536))
    for r in sorted(raws):
        assert table[r] == ar.lut_floor_exact(r, density_scale, n), (density_scale, r)
    assert table.min() >= -1 and table.max() <= n and (density_scale < 0 or np.all(np.diff(table) >= 0))


def test_distance_definition_equals_separable_construction():
    """The Chebyshev distance to the nearest non-empty cell, capped at 15, three ways on random small grids: every cell against every
    non-empty cell (the definition), the reference's clipped-cube counts, and the separable min-of-max passes the device builds it
    with -- which is therefore legitimate."""
    rs = np.random.RandomState(2)
    grids = [(1, 1, 1), (40, 1, 1), (1, 33, 2), (5, 3, 2), (19, 11, 5), (17, 18, 16), (36, 4, 3)]
    for gx, gy, gz in grids:
        for density in (0.0, 0.002, 0.02, 0.3, 1.0):
            ne = rs.rand(gz, gy, gx) < density
            if density == 0.002:
                ne[:] = False
                ne[gz - 1, gy - 1, gx - 1] = True                          # one cell in a corner: the longest distances
            brute = ar.chebyshev_distance_brute(ne)
            assert np.array_equal(ar.chebyshev_distance(ne), brute), (gx, gy, gz, density)
            assert np.array_equal(ar.chebyshev_distance_separable(ne), brute), (gx, gy, gz, density)
    assert ar.chebyshev_distance_brute(np.zeros((2, 2, 2), bool)).min() == ar.DIST_CAP


def test_packing_and_thresholds():
    bits = np.zeros(70, dtype=bool)
    bits[[0, 31, 32, 69]] = True
    assert ar.pack_bits(bits).tolist() == [0x80000001, 1, 1 << 5] and len(ar.pack_bits(bits, 10)) == 10
    assert ar.pack_nibbles(np.arange(10) + 1).tolist() == [0x87654321, 0xA9]
    thr = ar.class_thresholds()
    assert thr[0] == 0 and np.isinf(thr[15]) and thr[14] == f32(f32(0.5) * f32(1.41421356237)) and thr[13] == f32(0.5) and thr[1] == f32(2.0 ** -7)
    assert np.all(np.diff(thr) > 0)
    # the byte of a bound: no draw the byte culls ((x >> 24) > B) can be below the bound, and B is the smallest such byte
    b = np.array([0.0, 2.0 ** -33, 1e-9, 0.003, 0.25, 0.5, 0.70710677, 0.999, 1.0, 1.5, np.inf], dtype=np.float32)
    B = ar.bound_byte(b, np.zeros(len(b), bool)).astype(np.int64)
    for bi, Bi in zip(b, B):
        if Bi < 255:
            assert ar.word_to_uniform((Bi + 1) << 24) >= bi
        if Bi > 0:
            assert ar.word_to_uniform((Bi << 24) - 1) < bi or Bi == 255
    assert B[0] == 0 and B[4] == 63 and B[5] == 127 and B[-1] == 255 and B[-3] == 255
    assert ar.bound_byte(np.array([0.1], f32), np.array([True]))[0] == 255


# ------------------------------------------------------------------------------------------------ the reference against the oracle
def _scene(name, tf_name):
    vox, _ = ar.named_volume(name)
    tf, mo, ds = ar.transfer_functions()[tf_name]
    return scenes.Scene(name=f"{name}/{tf_name}", vox=vox, spacing=(1.0, 1.0, 1.0), max_magnitude=1.0, tf_rgba=tf, max_opacity=mo, width=8, height=8,
                        density_scale=ds)


def _points(rs, dim, shift, n):
    """Texture coordinates in [0, 1]^3: uniform ones, exact 0 and 1, and coordinates ON the boundaries between trilinear cells and
    between macro-cells (u N - 0.5 an integer, as nearly as float32 allows -- the fma decides the side)."""
    cols = []
    for N in dim:
        u = rs.rand(n)
        kind = rs.randint(0, 8, n)
        c = rs.randint(-1, N + 1, n)
        cell_edge = (c + 0.5) / N
        m = rs.randint(0, ((N - 1) >> shift) + 2, n)
        macro_edge = ((m << shift) - 0.5) / N                              # cell c + 1 = m S begins here
        u = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, np.where(kind == 2, cell_edge, np.where(kind == 3, macro_edge, u))))
        base = np.clip(u, 0.0, 1.0).astype(np.float32)
        nudge = rs.randint(-1, 2, n)                                       # the boundary itself, or one ulp either side of it
        on_edge = (kind == 2) | (kind == 3)
        u32 = np.where(on_edge & (nudge < 0), np.nextafter(base, f32(-1)), np.where(on_edge & (nudge > 0), np.nextafter(base, f32(2)), base))
        cols.append(np.clip(u32, f32(0), f32(1)).astype(np.float32))
    return np.stack(cols, axis=1)


def _cell_of(u, N):
    """c = floor(fma(u, N, -0.5)) as the sampler evaluates it (float64 product and sum are exact for a float32 u in [0, 1] and
    N < 2^24 unless u N < 2^-20, where the floor is -1 whatever the rounding; then one rounding to float32)."""
    return np.floor((u.astype(np.float64) * float(N) - 0.5).astype(np.float32)).astype(np.int64)


# every table on the small volumes; the flat volumes under the tables their GPU tests use
ANCHOR_CASES = [(v, t) for v in ar.SMALL_VOLUMES for t in ar.transfer_functions()] + [(v, t) for v in ar.FLAT_VOLUMES for t in ("default", "hazy")]


@pytest.mark.parametrize("name,tf_name", ANCHOR_CASES)
def test_reference_tables_bound_the_oracle(oracle, name, tf_name):
    """The anchor of the numpy reference: at random points of the texture domain -- with exact 0, 1 and cell boundaries -- the alpha
    the ORACLE's sampler and look-up return (svo_tex3d, x densityScale, svo_tex1d) is at most A(m) of the point's macro-cell (integer
    rule: c = floor(u N - 0.5), m = min((c + 1) >> shift, g - 1)), exactly 0 where the cell is `empty`, and at most the wide table's
    bound of every half-resolution cell whose one-voxel-wider footprint contains the point."""
    vox, vt = ar.named_volume(name)
    tf, mo, ds = ar.transfer_functions()[tf_name]
    T = ar.accel_tables(vt, tf, ds, mo)
    o = binding.OracleScene(_scene(name, tf_name))
    lib = o.lib
    rs = np.random.RandomState(ANCHOR_CASES.index((name, tf_name)))
    n = 6000
    P = _points(rs, vt.dim, vt.shift, n)
    rgba = (C.c_float * 4)()
    alpha = np.empty(n, dtype=np.float32)
    dsf = f32(ds)
    for i in range(n):
        I = f32(lib.svo_tex3d(o.ptr, C.c_float(P[i, 0]), C.c_float(P[i, 1]), C.c_float(P[i, 2]))) * dsf
        lib.svo_tex1d(o.ptr, C.c_float(I), rgba)
        alpha[i] = rgba[3]
    c = [_cell_of(P[:, a], vt.dim[a]) for a in range(3)]
    for a in range(3):
        assert c[a].min() >= -1 and c[a].max() <= vt.dim[a] - 1
    m = [np.minimum((c[a] + 1) >> vt.shift, vt.grid[a] - 1) for a in range(3)]
    A = T.A[m[2], m[1], m[0]]
    nan = np.isnan(alpha)
    ok = (alpha <= A) | (nan & np.isinf(A))
    assert ok.all(), f"{np.count_nonzero(~ok)} points above their cell's bound, e.g. {P[~ok][0]}: alpha {alpha[~ok][0]} > A {A[~ok][0]}"
    e = T.empty[m[2], m[1], m[0]]
    assert np.all(alpha[e] == 0), f"non-zero alpha in an `empty` cell at {P[e][alpha[e] != 0][:1]}"
    # the wide table: half-resolution cells of 2 S voxels whose footprint, one voxel wider, holds the point's trilinear cell
    S2 = 2 << vt.shift
    cand = []
    for a in range(3):
        h0 = np.minimum((c[a] + 1) // S2, vt.hgrid[a] - 1)
        lst = []
        for d in (-1, 0, 1):
            h = h0 + d
            valid = (h >= 0) & (h < vt.hgrid[a]) & (h * S2 - 1 <= c[a] + 1) & ((c[a] + 1 <= h * S2 + S2) | (h == vt.hgrid[a] - 1))
            lst.append((np.clip(h, 0, vt.hgrid[a] - 1), valid))
        cand.append(lst)
    tested = 0
    for hz, vz in cand[2]:
        for hy, vy in cand[1]:
            for hx, vx in cand[0]:
                v = vx & vy & vz
                Aw = T.A_wide[hz, hy, hx]
                okw = ~v | (alpha <= Aw) | (nan & np.isinf(Aw))
                assert okw.all(), f"{np.count_nonzero(~okw)} points above a wide cell's bound, e.g. {P[~okw][0]}"
                tested += int(v.sum())
    assert tested > n                                                      # (most points lie in one wide cell, those near a boundary in more)
    if tf_name not in ("transparent", "negative_scale"):                   # (a negative scale maps every voxel to the table's first entry: alpha 0)
        assert (alpha[~nan] > 0).any()


# ------------------------------------------------------------------------------------------------ non-vacuity
# What each volume must show under the DEFAULT table (the other tables of the GPU tests vary the bounds on the same grids): everything
# below, for every volume, with exactly these exceptions, which the prescribed shapes make impossible:
#  * a distance of 15 next to a non-empty cell needs 16 cells on one axis: the 10 x 6 x 3 and 5 x 3 x 2 grids of 37 x 21 x 10 at shift 2
#    and 3 cannot hold one;
#  * the single non-zero voxel of 40 x 8 x 8 lies in cells of one and the same maximum: exactly one class between 1 and 14.
# One more concerns the HALF-resolution nibble only, not the distance: in the 19 x 11 x 5 grid of shift 1 the full-resolution distance
# reaches 15 (asserted), but a nibble of 15 needs cells 0 AND 1 at 15, i.e. no non-zero voxel below x = 32; the 3 x 2 x 1 half-resolution
# grid of shift 3 then keeps a single x cell (voxels 31 .. 39) for all structure, dense or not, and cannot show two middle classes next to
# the dense structure the same volume must have.  The two middle classes at shift 3 were kept.
NO_DIST_CAP = {"37x21x10_s2", "37x21x10_s3"}
NO_HALF_RES_CAP = NO_DIST_CAP | {"37x21x10_s1"}
MIN_MID_CLASSES = {"40x8x8_s0": 1}


def _edge_limited(T):
    """cells whose distance is limited by the grid's end: the all-empty cube of radius D - 1 around them reaches beyond the grid"""
    gz, gy, gx = T.dist.shape
    z, y, x = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    to_edge = np.minimum.reduce([x, gx - 1 - x, y, gy - 1 - y, z, gz - 1 - z])
    return T.dist.astype(np.int64) - 1 > to_edge


@pytest.mark.parametrize("name", list(ar.VOLUMES))
def test_reference_tables_are_not_vacuous(name):
    vox, vt = ar.named_volume(name)
    tf, mo, ds = ar.transfer_functions()["default"]
    T = ar.accel_tables(vt, tf, ds, mo)
    assert T.empty.any() and not T.empty.all()
    assert T.deep.any() and (T.empty & ~T.deep).any()
    assert _edge_limited(T).any()
    if name not in NO_DIST_CAP:
        assert T.dist.max() == ar.DIST_CAP
    else:
        assert max(vt.grid) < 16 and 2 <= T.dist.max() < ar.DIST_CAP
    assert (T.hdist == ar.DIST_CAP).any() == (name not in NO_HALF_RES_CAP)
    assert set(np.unique(T.dist).tolist()) >= set(range(min(int(T.dist.max()), 4) + 1))          # every distance from 0 up
    mid = [c for c in np.unique(T.hcls).tolist() if 1 <= c <= 14]
    assert (T.hcls == 0).any() and len(mid) >= MIN_MID_CLASSES.get(name, 2), np.unique(T.hcls)
    assert T.census[0] > 0 and T.census[2] == int(T.empty.sum())
    # the volume itself: exact-zero air, a non-zero last voxel on every axis, odd children beyond the grid's end where the grid is odd
    assert (vox == 0).any() and vox[-1, -1, -1] != 0
    if vt.fgrid is not None:
        assert T.sub8 is not None and 0 < np.unique(T.sub8).size and (T.sub8 == 0).any() and (T.sub8 == 255).any()
    assert (T.bnd8 is None) == (name in ar.FLAT_VOLUMES)


def test_reference_tables_cover_every_class_and_many_bytes():
    """Across the tables of the GPU tests: class 15 from a bound of 1 AND from an entry that is not a number, at least 8 distinct
    bound bytes below 255 in one table, grids with odd dimensions at full and at half resolution, a wide table whose ring matters."""
    tfs = ar.transfer_functions()
    _, vt = ar.named_volume("64_s1")
    hazy = ar.accel_tables(vt, *[tfs["hazy"][i] for i in (0, 2, 1)])
    byts = np.unique(hazy.bnd8[: ar.BOUND8_DIM ** 3])
    assert np.count_nonzero(byts < 255) >= 8, byts
    assert len([c for c in np.unique(hazy.hcls) if 1 <= c <= 14]) >= 6 and not hazy.empty.any()
    nan = ar.accel_tables(vt, *[tfs["nan_alpha"][i] for i in (0, 2, 1)])
    dflt = ar.accel_tables(vt, *[tfs["default"][i] for i in (0, 2, 1)])
    assert np.isinf(nan.A).any() and nan.census[1] > dflt.census[1] > 0 and (nan.bnd8[: ar.BOUND8_DIM ** 3] == 255).sum() > (dflt.bnd8[: ar.BOUND8_DIM ** 3] == 255).sum()
    assert ar.accel_tables(vt, *[tfs["transparent"][i] for i in (0, 2, 1)]).empty.all()
    op = ar.accel_tables(vt, *[tfs["opaque"][i] for i in (0, 2, 1)])
    assert not op.empty.any() and op.dist.max() == 0
    _, v37 = ar.named_volume("37x21x10_s0")
    assert all(g % 2 == 1 for g in v37.grid[:2]) and v37.hgrid == (19, 11, 5)
    assert ar.accel_tables(v37, *[tfs["negative_scale"][i] for i in (0, 2, 1)]).empty.all()      # every look-up clamps to the first entry, alpha 0
    for name in ar.FLAT_VOLUMES:
        _, vt = ar.named_volume(name)
        psh, pg = _parent_rule(*vt.dim, 0)
        assert vt.shift == psh + 1 and ar.ceil_div(np.prod([(c + 1) // 2 for c in pg]), 8) > ar.DIST_WORDS_MAX >= ar.ceil_div(int(np.prod(vt.hgrid)), 8)
