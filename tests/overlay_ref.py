"""Test-side reference of the overlay calls (include/svr_abi.h, "overlays"), numpy only and literal.  The sample points of a slice are
those of tests/slice_ref.py (Reference.points); the voxel of a point is svr_region_seed_from_world's mapping with the product in float64,
where it is exact; ids, edges and the blend are the header's definitions in integers.

It also holds the fixtures that tests/test_overlay_cpu.py (their conditions, on the reference alone) and tests/test_overlay_gpu.py (the
comparisons) share: scenes, sources, planes, windows, palettes."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from sunvolumerender_amd import abi, host, scenes
from tests import geodesic_ref as gr
from tests import label_ref as lr
from tests import region_ref as rr
from tests import slice_ref as sr

f32 = np.float32
FOUND = 2                                   # SVR_HIT_STATUS_FOUND
NONE_ID = np.uint64(1) << np.uint64(32)     # larger than every id: "no non-zero id yet"


# ------------------------------------------------------------------------------------------------ the definitions
def voxel_ids(vol, source, P):
    """ids (uint32, P.shape[:-1]) of the float32 points P[..., 3]: VOXEL OF A POINT, then the source's value there.  source: a bool mask
    or a uint32 label array [nz][ny][nx]."""
    P = np.asarray(P, dtype=np.float32)
    dims = source.shape[::-1]                                         # nx, ny, nz
    ok = np.ones(P.shape[:-1], dtype=bool)
    idx = []
    with np.errstate(all="ignore"):
        for a, name in enumerate("xyz"):
            d = P[..., a] - f32(getattr(vol.bbox.vmin, name))
            tc = d * f32(getattr(vol.bbox.invSize, name))
            assert d.dtype == tc.dtype == np.float32
            good = (tc >= 0) & (tc <= 1)                              # (NaN compares false)
            ok &= good
            i = np.floor(np.where(good, tc, 0).astype(np.float64) * float(dims[a])).astype(np.int64)     # exact: 24 x 31 bits
            idx.append(np.minimum(i, dims[a] - 1))                    # the far face belongs to the last voxel
    ids = np.asarray(source)[idx[2], idx[1], idx[0]].astype(np.uint32)
    return np.where(ok, ids, np.uint32(0))


def slice_ids(R: sr.Reference, p, w, h, source, k=0, spacing=0.0, want_centre=False):
    """ID OF A SLICE PIXEL for every pixel of slice k: (ids[h, w] uint32, counting[h, w] = the number of counting samples); with
    want_centre also the ids of the same plane without its thickness."""
    P, inside = R.points(p, w, h, k, spacing)
    ids = voxel_ids(R.vol, source, P).astype(np.uint64)
    cand = np.where(inside & (ids != 0), ids, NONE_ID)
    best = cand.min(axis=0)
    out = np.where(best == NONE_ID, 0, best).astype(np.uint32)
    if not want_centre:
        return out, inside.sum(axis=0)
    q = abi.SliceParams.from_buffer_copy(p)
    q.thickness = 0.0
    return out, inside.sum(axis=0), slice_ids(R, q, w, h, source, k, spacing)[0]


def hit_ids(vol, source, hits):
    """ID OF A HIT PIXEL for an array of host.HIT_DTYPE records."""
    ids = voxel_ids(vol, source, hits["position"])
    return np.where(hits["status"] == FOUND, ids, np.uint32(0))


def edges(ids):
    """EDGE for id images [..., h, w]: a bool array of the same shape."""
    ids = np.asarray(ids)
    e = np.zeros(ids.shape, dtype=bool)
    e[..., :, 1:] |= ids[..., :, 1:] != ids[..., :, :-1]
    e[..., :, :-1] |= ids[..., :, :-1] != ids[..., :, 1:]
    e[..., 1:, :] |= ids[..., 1:, :] != ids[..., :-1, :]
    e[..., :-1, :] |= ids[..., :-1, :] != ids[..., 1:, :]
    return e & (ids != 0)


def unpack_palette(palette):
    """[n][4] int64 (r, g, b, a) of uint32 RGBA8 entries with r in the low byte."""
    pal = np.asarray(palette, dtype=np.uint32).astype(np.int64)
    return np.stack([pal & 255, (pal >> 8) & 255, (pal >> 16) & 255, (pal >> 24) & 255], axis=-1)


def blend(img, ids, palette, fill_alpha, edge_alpha):
    """BLEND of RGBA8 images [..., h, w, 4] by their id images: a new array."""
    pal = unpack_palette(palette)
    ids = np.asarray(ids)
    on = ids != 0
    e = pal[(ids.astype(np.int64) - 1) % len(pal)]                     # (any entry where id == 0: masked below)
    A = np.where(edges(ids), int(edge_alpha), int(fill_alpha))
    a = (A * e[..., 3] + 127) // 255
    write = on & (a != 0)
    out = np.array(img, dtype=np.uint8, copy=True)
    rgb = out[..., :3].astype(np.int64)
    new = (rgb * (255 - a[..., None]) + e[..., :3] * a[..., None] + 127) // 255
    out[..., :3] = np.where(write[..., None], new, rgb).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ fixtures
BRAIN_WINDOW = (23593, 28835)            # BRAIN of tests/test_region_cpu.py
NOISY_WINDOW = (24500, 27500)            # of tiny_head_noisy: a narrow window, so the noise tears the tissue into many small parts
SPLIT_R2 = 4
SKIN = 3000                              # the head from the outermost skin voxels inwards: the ray caster turns opaque about there
HIT_SOURCES = ("head mask", "octants")
HIT_MODES = ((1, 0.5, 0.45, "opacity"), (2, 0.5, 0.45, "iso"))      # SVR_HIT_OPACITY / SVR_HIT_ISO, alpha, iso
IMAGES = ((96, 80), (27, 19))            # tiny_head's own size, and one with partly empty tiles
SLAB = (5.0, 0.625)                      # thickness, step: K = 9
STACK = (3, 2.5)                         # count, spacing
CROP = (slice(17, 30), slice(14, 35), slice(5, 42))    # nz, ny, nx = 13, 21, 37

CUSTOM_PALETTE = np.array([0xFF2010F0, 0x00FFFFFF, 0x8000C8FF, 0xFFFFFFFF, 0xFF000000], dtype=np.uint32)   # one of alpha 0, one of alpha 128


def scene(name):
    """'head': tiny_head (48^3: wx = 2, 16 padding bits per row); 'crop': a 37 x 21 x 13 crop of it (27 padding bits)."""
    def make():
        sc = scenes.make_scene("tiny_head")
        if name == "crop":
            sc = scenes.make_scene("tiny_head", vox=np.ascontiguousarray(sc.vox[CROP]))
        return sc
    return rr.cached(("overlay scene", name), make)


def reference(name) -> sr.Reference:
    return sr.reference(("overlay", name), lambda: scene(name))


def source(name):
    """The id volume of a named source, as the numpy references of the region calls give it (the GPU tests take theirs from the device
    calls and compare).  'mask': the brain window (bool); 'labels6': the parts of the noisy window under connectivity 6; 'zones': the
    zones of the brain window's split; 'patched': labels6 with 0xFFFFFFFF and ids above every palette; 'crop mask': the brain window of
    the crop.  For the 3D views, whose rays stop at the skin: 'head mask' (everything from the skin inwards) and 'octants' (the same,
    labelled 1 .. 8 by octant)."""
    def make():
        head = scene("head").vox
        if name == "mask":
            return lr.threshold(head, *BRAIN_WINDOW)
        if name == "crop mask":
            return lr.threshold(scene("crop").vox, *BRAIN_WINDOW)
        if name == "labels6":
            return lr.label(noisy_mask(), 6)[0]
        if name == "zones":
            return gr.split(necked_mask(), SPLIT_R2, 26)[0]
        if name == "patched":
            return patch_labels(source("labels6"))
        if name == "head mask":
            return head >= SKIN
        if name == "octants":
            z, y, x = np.indices(head.shape)
            return np.where(head >= SKIN, 1 + (x >= 24) + 2 * (y >= 20) + 4 * (z >= 24), 0).astype(np.uint32)
        raise KeyError(name)
    return rr.cached(("overlay source", name), make)


def noisy_mask():
    return lr.threshold(scenes.make_scene("tiny_head_noisy").vox, *NOISY_WINDOW)


def necked_mask():
    """The brain window cut into eight lobes by three slabs of three voxels, with a 3 x 3 neck left through every slab face between
    two lobes: the erosion of the split removes the necks, so its zones are the lobes."""
    cut = np.zeros((48, 48, 48), dtype=bool)
    neck = np.zeros_like(cut)
    lobes = (slice(15, 18), slice(30, 33))
    for a in range(3):
        sl = [slice(None)] * 3
        sl[a] = slice(22, 25)
        cut[tuple(sl)] = True
        for i in lobes:
            for j in lobes:
                sl2 = [i, j]
                sl2.insert(a, slice(22, 25))
                neck[tuple(sl2)] = True
    return source("mask") & (~cut | neck)


def patch_labels(labels):
    """every third label becomes 0xFFFFFFFF, every third one 1000 + itself: ids beyond every palette_count"""
    out = labels.copy()
    out[(labels % 3) == 1] = 0xFFFFFFFF
    sel = (labels % 3) == 2
    out[sel] = labels[sel] + 1000
    return out


def scene_of(source_name):
    return "crop" if source_name.startswith("crop") else "head"


def planes(name, w, h):
    """(name, params) of test_slice_gpu.py's planes() for the scene at w x h, without a device: three axis planes, two oblique ones."""
    from tests import test_slice_gpu as tsg
    lib, R, sc = abi.load(), reference(name), scene(name)
    rig = SimpleNamespace(canvas=SimpleNamespace(slice_params_axis=lambda axis, pos: host.slice_params_axis(lib, R.vol, axis, pos, w, h)),
                          sc=sc, W=w, dev=SimpleNamespace(lib=lib))
    return tsg.planes(rig, 1.0)


def slab(p):
    q = abi.SliceParams.from_buffer_copy(p)
    q.thickness, q.step = SLAB
    return q


def window_of(w, h):
    """a render window with odd offsets"""
    return (w // 4 | 1, h // 4 | 1, (3 * w // 4) | 1, (3 * h // 4) | 1)


def cut_out(full, base, win, channels=True):
    """`base` with the window's pixels taken from `full`: images [..., h, w, 4], or id images [..., h, w] with channels=False"""
    x0, y0, x1, y1 = win
    out = base.copy()
    if channels:
        out[..., y0:y1, x0:x1, :] = full[..., y0:y1, x0:x1, :]
    else:
        out[..., y0:y1, x0:x1] = full[..., y0:y1, x0:x1]
    return out


def shard_rows(h, strip, rank, world):
    """the rows y of an image of height h that rank owns: (y // strip) % world == rank, svr_set_row_shard's rule"""
    return (np.arange(h) // strip) % world == rank


def seam(ids, m):
    """does an id boundary lie on a tile seam of m pixels in x AND in y: two neighbours with different ids, the second at a multiple of m"""
    dx, dy = ids[:, 1:] != ids[:, :-1], ids[1:, :] != ids[:-1, :]
    return bool(dx[:, m - 1::m].any()) and bool(dy[m - 1::m, :].any())


def crosses_window(ids, win):
    """does an id boundary lie on the border of the window: a pixel inside and its neighbour outside with different ids"""
    x0, y0, x1, y1 = win
    dx, dy = ids[:, 1:] != ids[:, :-1], ids[1:, :] != ids[:-1, :]
    return bool(dx[y0:y1, x0 - 1].any() or dx[y0:y1, x1 - 1].any() or dy[y0 - 1, x0:x1].any() or dy[y1 - 1, x0:x1].any())


SOURCES = ("mask", "labels6", "zones", "patched", "crop mask")


def cases(source_name, w, h):
    """(what, params) of the slice geometries every slice test runs for a source at w x h: the five planes, each as a plane and as a slab"""
    out = []
    for pname, p in planes(scene_of(source_name), w, h):
        out.append((f"{source_name} {w}x{h} {pname} plane", p))
        out.append((f"{source_name} {w}x{h} {pname} slab", slab(p)))
    return out
