"""svr_region_grow / _stats_of / _apply on the GPU: the whole mask -- as uint32 words, padding included -- and every integer of the
statistics are EQUAL to the test-side reference (tests/region_ref.py: a numpy fixpoint iteration and literal statistics).  The fixtures
and the conditions they meet are those of tests/test_region_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from sunvolumerender_amd import abi, host, scenes
from tests import region_ref as rr
from tests.test_region_cpu import BONE, BRAIN, THIN, bone_seed

pytestmark = pytest.mark.gpu

CONNS = (6, 18, 26)


class Grower:
    """Raw calls with a mask buffer the test owns: returns the status, the mask words and the statistics."""

    def __init__(self, dev):
        self.dev, self.lib = dev, dev.lib

    def grow(self, vox, seeds, lo, hi, conn=6, box=None, max_sweeps=0, on_device=False, prefill=0xFF):
        dev = self.dev
        vox = np.ascontiguousarray(vox, dtype=np.uint16)
        nz, ny, nx = vox.shape
        words = host.region_mask_words(vox.shape)
        mask = dev.malloc(4 * words)
        src = None
        try:
            dev.check(self.lib.svr_memset_device(C.c_void_p(mask), prefill, 4 * words))       # the call overwrites whatever is there
            if on_device:
                src = dev.malloc(vox.nbytes)
                dev.to_device(src, vox)
            p = dev.region_params(lo, hi, conn, box, max_sweeps)
            xyz = np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
            st = abi.RegionStats()
            rc = self.lib.svr_region_grow(C.c_void_p(src) if on_device else vox.ctypes.data_as(C.c_void_p), nx, ny, nz, 1 if on_device else 0,
                                          xyz.ctypes.data_as(C.POINTER(C.c_int32)), len(xyz), C.byref(p), C.c_void_p(mask), C.byref(st))
            msg = self.lib.svr_last_error().decode()
            self.lib.svr_clear_error()
            return rc, dev.to_host(mask, (words,), np.uint32), st, msg
        finally:
            dev.free(mask)
            if src is not None:
                dev.free(src)


def same_stats(st, ref, what):
    got = st.as_dict()
    for k in rr.STAT_INTS:
        assert got[k] == ref[k], f"{what}: {k} is {got[k]}, reference {ref[k]}"


def check(dev, name, vox, seeds, lo, hi, conn=6, box=None, **kw):
    """One grow against the reference: words and statistics; returns (words, stats, reference region)."""
    region, ref = rr.reference(name, vox, seeds, lo, hi, conn, box)
    rc, words, st, msg = Grower(dev).grow(vox, seeds, lo, hi, conn, box, **kw)
    what = f"{name} {vox.shape} window {lo}..{hi} conn {conn}"
    assert rc == 0, f"{what}: {rc} {msg}"
    want = rr.pack(region)
    if not np.array_equal(words, want):
        diff = rr.unpack(words ^ want, vox.shape)
        first = np.argwhere(diff)[:1]
        raise AssertionError(f"{what}: {int(diff.sum())} voxels differ (got {int(rr.unpack(words, vox.shape).sum())}, reference "
                             f"{int(region.sum())}); first (z, y, x) {first.tolist()}; padding differs: {not np.array_equal(rr.pack(rr.unpack(words, vox.shape)), words)}")
    same_stats(st, ref, what)
    cap = dev.lib.svr_region_default_max_sweeps(vox.shape[2], vox.shape[1], vox.shape[0])
    assert 1 <= st.sweeps <= cap
    return words, st, region


@pytest.fixture(scope="module")
def head():
    return scenes.make_scene("tiny_head").vox


# ------------------------------------------------------------------------------------------------ the tiny_head volume (48^3)
@pytest.mark.parametrize("conn", CONNS)
def test_head_brain_bone_thin(hip_dev, head, conn):
    for lo, hi, seed, sizes, _ in (BRAIN, BONE, THIN):
        seed = bone_seed(head) if seed is None else seed
        _, st, _ = check(hip_dev, "head", head, [seed], lo, hi, conn)
        assert st.voxels == sizes[conn]


def test_head_air_whole_and_noisy(hip_dev, head):
    _, st, _ = check(hip_dev, "head", head, [(0, 0, 0)], 0, 0, 6)
    assert st.voxels == 74800 and list(st.bbox_min) == [0, 0, 0] and list(st.bbox_max) == [47, 47, 47]
    _, st, _ = check(hip_dev, "head", head, [(7, 8, 9)], 0, 65535, 6)
    assert st.voxels == head.size
    noisy = scenes.make_scene("tiny_head_noisy").vox
    _, st, _ = check(hip_dev, "noisy", noisy, [(0, 0, 0)], 0, 300, 6)
    assert st.voxels == 76205


# ------------------------------------------------------------------------------------------------ kernel edge cases
@pytest.mark.parametrize("shape", rr.EDGE_SHAPES, ids=lambda s: "x".join(str(n) for n in s[::-1]))
def test_shapes(hip_dev, shape):
    vox = rr.noise_volume(shape)
    seeds = rr.spread_seeds(vox)
    for conn in CONNS:
        check(hip_dev, "noise", vox, seeds, rr.NOISE_LO, rr.NOISE_HI, conn)
    check(hip_dev, "noise", vox, seeds, rr.NOISE_LO, rr.NOISE_HI, 6, on_device=True)          # (the 16-byte path where nx % 8 == 0)


@pytest.mark.parametrize("name, a, b", rr.PAIRS, ids=[p[0] for p in rr.PAIRS])
def test_pairs_across_boundaries(hip_dev, name, a, b):
    vox = rr.pair_volume(a, b)
    for conn in CONNS:
        for s, o in ((a, b), (b, a)):
            _, st, _ = check(hip_dev, "pair" + name, vox, [s], 1000, 1000, conn)
            assert st.voxels == rr.pair_expected(s, o, conn)


def test_seeds_at_the_eight_corners(hip_dev):
    vox = rr.noise_volume((10, 10, 130)).copy()
    nz, ny, nx = vox.shape
    corners = [(x, y, z) for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)]
    for x, y, z in corners:
        vox[z, y, x] = 0
    for conn in CONNS:
        _, st, region = check(hip_dev, "corners", vox, corners, rr.NOISE_LO, rr.NOISE_HI, conn)
        assert all(region[z, y, x] for x, y, z in corners)


def test_serpentine_needs_many_sweeps_and_the_cap_is_an_error(hip_dev):
    vox, seed = rr.serpentine()
    nz, ny, nx = vox.shape
    cap = hip_dev.lib.svr_region_default_max_sweeps(nx, ny, nz)
    _, st, region = check(hip_dev, "serpentine", vox, [seed], 1000, 1000, 6)
    assert 1 < st.sweeps <= cap and st.voxels == int((vox == 1000).sum())
    print(f"serpentine: {st.sweeps} sweeps of at most {cap}")
    rc, words, st2, msg = Grower(hip_dev).grow(vox, [seed], 1000, 1000, 6, max_sweeps=2)
    assert rc == abi.REGION_ERR_SWEEPS and "sweeps" in msg and "svr_region_grow" in msg and st2.sweeps == 2
    part = rr.unpack(words, vox.shape)
    assert part[0, 0, 0] and not (part & ~region).any() and part.sum() < region.sum()       # a part of the region, never more
    # the same volume once more with the default cap: the error left nothing behind
    check(hip_dev, "serpentine", vox, [seed], 1000, 1000, 6)


def test_seed_handling(hip_dev):
    vox = rr.noise_volume((12, 20, 70), seed=11)
    rng = np.random.default_rng(5)
    seeds = [tuple(int(rng.integers(0, n)) for n in (70, 20, 12)) for _ in range(56)]
    seeds = seeds + seeds[:8]                                                               # 64 seeds, 8 of them twice
    cand = rr.candidates(vox, rr.NOISE_LO, rr.NOISE_HI)
    assert len(seeds) == abi.REGION_MAX_SEEDS and 0 < sum(1 for x, y, z in seeds if not cand[z, y, x]) < 56
    for conn in CONNS:
        check(hip_dev, "seeds64", vox, seeds, rr.NOISE_LO, rr.NOISE_HI, conn)
    # two seeds in two components
    two = np.zeros((9, 12, 40), dtype=np.uint16)
    two[1:4, 2:6, 3:9] = 700
    two[5:8, 7:11, 30:38] = 700
    for seeds2, n in (([(4, 3, 2)], 72), ([(4, 3, 2), (33, 8, 6)], 72 + 96)):
        _, st, _ = check(hip_dev, "two", two, seeds2, 700, 700, 26)
        assert st.voxels == n
    # no seed is a candidate: EMPTY, not an error
    rc, words, st, _ = Grower(hip_dev).grow(two, [(0, 0, 0), (20, 6, 4)], 700, 700, 6)
    assert rc == 0 and st.status == abi.REGION_STATUS_EMPTY and st.voxels == 0 and not words.any()
    assert list(st.bbox_min) == [40, 12, 9] and list(st.bbox_max) == [-1, -1, -1] and (st.vmin, st.vmax) == (65535, 0)
    same_stats(st, rr.stats(two, np.zeros(two.shape, dtype=bool)), "empty")


def test_box_cuts_a_region(hip_dev):
    vox, seed, box = rr.bridge_volume()
    _, whole, _ = check(hip_dev, "bridge", vox, [seed], 500, 500, 6)
    _, cut, region = check(hip_dev, "bridge", vox, [seed], 500, 500, 6, box)
    assert cut.voxels < whole.voxels and not region[:, :, 30:].any()
    nv = rr.noise_volume((9, 10, 37))
    for conn in CONNS:
        check(hip_dev, "noisebox", nv, rr.spread_seeds(nv), rr.NOISE_LO, rr.NOISE_HI, conn, ((2, 1, 0), (30, 8, 7)))
    # a seed outside the box is not a candidate
    rc, words, st, _ = Grower(hip_dev).grow(vox, [(32, 3, 4)], 500, 500, 6, ((0, 0, 0), (20, 19, 9)))
    assert rc == 0 and st.status == abi.REGION_STATUS_EMPTY and not words.any()


def test_host_and_device_sources_prefill_and_no_state(hip_dev, head):
    g = Grower(hip_dev)
    a = g.grow(head, [BRAIN[2]], BRAIN[0], BRAIN[1], 6, on_device=False, prefill=0xFF)
    b = g.grow(head, [BRAIN[2]], BRAIN[0], BRAIN[1], 6, on_device=True, prefill=0x00)
    assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1]) and a[2].as_dict() == b[2].as_dict()
    # two calls in a row with different windows, then the first again
    first = check(hip_dev, "head", head, [BRAIN[2]], BRAIN[0], BRAIN[1], 6)[0]
    check(hip_dev, "head", head, [bone_seed(head)], BONE[0], BONE[1], 6)
    again = check(hip_dev, "head", head, [BRAIN[2]], BRAIN[0], BRAIN[1], 6)[0]
    assert np.array_equal(first, again) and np.array_equal(first, a[1])
    # the Python layer returns the same region
    mask, st = hip_dev.region_grow(head, [BRAIN[2]], BRAIN[0], BRAIN[1])
    assert mask.dtype == bool and mask.shape == head.shape and np.array_equal(rr.pack(mask), first) and st.voxels == BRAIN[3][6]
    m = hip_dev.region_measure(st, (0.5, 1.0, 2.0))
    want = rr.measure(head, mask, (0.5, 1.0, 2.0))
    assert m.volume == pytest.approx(want["volume"], rel=1e-13) and m.stddev == pytest.approx(want["stddev"], rel=1e-9)


# ------------------------------------------------------------------------------------------------ svr_region_stats_of
def test_stats_of(hip_dev, head):
    region, ref = rr.reference("head", head, [BRAIN[2]], BRAIN[0], BRAIN[1], 6)
    st = hip_dev.region_stats_of(head, region)
    same_stats(st, ref, "stats of the grown mask")
    assert st.sweeps == 0
    # hand-made masks: a box with a hole that touches the volume's faces; single voxels at both ends of a word; all; none
    for shape in ((9, 10, 70), (5, 8, 64)):
        vox = rr.noise_volume(shape, seed=3)
        hand = np.zeros(shape, dtype=bool)
        hand[0:6, 2:, 20:50] = True
        hand[2:4, 4:6, 30:40] = False
        hand[-1, -1, -1] = hand[0, 0, 0] = hand[3, 0, 31] = hand[3, 0, 32] = True
        for mask in (hand, np.ones(shape, dtype=bool), np.zeros(shape, dtype=bool)):
            same_stats(hip_dev.region_stats_of(vox, mask), rr.stats(vox, mask), f"hand-made mask {shape}")
        buf = hip_dev.malloc(vox.nbytes)
        try:
            hip_dev.to_device(buf, vox)
            same_stats(hip_dev.region_stats_of(buf, hand, shape=shape), rr.stats(vox, hand), "device source")
        finally:
            hip_dev.free(buf)


# ------------------------------------------------------------------------------------------------ svr_region_apply
@pytest.mark.parametrize("shape", [(48, 48, 48), (5, 7, 33)], ids=["48x48x48", "33x7x5"])
def test_apply(hip_dev, head, shape):
    if shape == (48, 48, 48):
        vox, (region, _) = head, rr.reference("head", head, [BRAIN[2]], BRAIN[0], BRAIN[1], 6)
    else:
        vox = rr.noise_volume(shape)
        region, _ = rr.reference("noise", vox, rr.spread_seeds(vox), rr.NOISE_LO, rr.NOISE_HI, 6)
    assert 0 < region.sum() < vox.size
    buf = hip_dev.malloc(vox.nbytes)
    try:
        for mode in (abi.REGION_KEEP, abi.REGION_REMOVE):
            for fill in (0, 1000):
                want = rr.apply(vox, region, mode, fill)
                assert np.array_equal(hip_dev.region_apply(vox, region, mode, fill), want)                   # host source
                hip_dev.to_device(buf, vox)
                assert np.array_equal(hip_dev.region_apply(buf, region, mode, fill, shape=shape), want)      # device, not aliased
                assert np.array_equal(hip_dev.to_host(buf, shape, np.uint16), vox)
                assert hip_dev.region_apply(buf, region, mode, fill, shape=shape, out_ptr=buf) == buf        # aliased
                assert np.array_equal(hip_dev.to_host(buf, shape, np.uint16), want)
    finally:
        hip_dev.free(buf)


# ------------------------------------------------------------------------------------------------ the loop, once
def _raycast(canvas, volume):
    dev = canvas.dev
    dev.check(dev.lib.svr_memset_device(C.c_void_p(canvas.img), 0, canvas.W * canvas.H * 4))
    dev.lib.render_raycasting(C.c_void_p(canvas.img), C.byref(volume), C.byref(canvas.transferFunction), C.byref(canvas.camera),
                              C.c_float(canvas.stepSize))
    dev.check()
    dev.synchronize()
    return canvas.read_img()


def test_pick_segment_measure_show(hip_dev, head):
    dev, lib = hip_dev, hip_dev.lib
    sc = scenes.make_scene("tiny_head")
    cv = host.Canvas(dev, sc.width, sc.height)
    scenes.apply_to_canvas(sc, cv)
    nz, ny, nx = head.shape
    d_out, texs = dev.malloc(head.nbytes), []
    try:
        before = _raycast(cv, cv.deviceVolume)
        # pick: the isosurface of bone through the image centre
        iso = 0.65                                      # (the centre ray never reaches 0.7: checked on the hit reference)
        hit = cv.pick([(sc.width // 2, sc.height // 2)], abi.HIT_ISO, iso=iso)[0]
        assert hit["status"] == abi.HIT_STATUS_FOUND
        seed = host.region_seed_from_world(lib, cv.deviceVolume, (nx, ny, nz), hit["position"])
        assert head[seed[2], seed[1], seed[0]] >= BONE[0], (seed, int(head[seed[2], seed[1], seed[0]]))
        # segment and measure
        mask, st = dev.region_grow(head, [seed], BONE[0], BONE[1])
        region, ref = rr.reference("head", head, [seed], BONE[0], BONE[1], 6)
        assert np.array_equal(mask, region) and st.voxels == 5410
        same_stats(st, ref, "bone from the pick")
        # show: the kept volume stays on the device and becomes a texture
        assert dev.region_apply(head, mask, abi.REGION_KEEP, 0, out_ptr=d_out) == d_out
        shown = []
        for voxels, on_device in ((C.c_void_p(d_out), 1), (np.ascontiguousarray(rr.apply(head, region, rr.KEEP, 0)), 0)):
            src = voxels if on_device else voxels.ctypes.data_as(C.c_void_p)
            tex = lib.svr_create_volume_texture(src, nx, ny, nz, on_device, abi.LAYOUT_AUTO)
            dev.check()
            texs.append(tex)
            vol = abi.cudaVolume.from_buffer_copy(cv.deviceVolume)
            vol.tex = tex
            shown.append(_raycast(cv, vol))
        assert np.array_equal(shown[0], shown[1])
        assert not np.array_equal(shown[0], before) and shown[0].any()
        # the region calls left the renderers alone
        assert np.array_equal(_raycast(cv, cv.deviceVolume), before)
    finally:
        for t in texs:
            lib.svr_destroy_texture(t)
        dev.free(d_out)
        cv.close()


# ------------------------------------------------------------------------------------------------ refusals with the device up
def test_refusals_leave_the_mask_alone(hip_dev):
    dev, lib = hip_dev, hip_dev.lib
    vox = rr.noise_volume((4, 4, 40))
    words = host.region_mask_words(vox.shape)
    mask = dev.malloc(4 * words)
    try:
        dev.check(lib.svr_memset_device(C.c_void_p(mask), 0xAB, 4 * words))
        st = abi.RegionStats()
        xyz = (C.c_int32 * 3)(0, 0, 0)
        for change, code in ((dict(connectivity=8), -3), (dict(lo=5, hi=4), -3), (dict(hi=70000), -3), (dict(box=((3, 0, 0), (2, 3, 3))), -3)):
            p = dev.region_params(**{**dict(lo=0, hi=100), **change})
            assert lib.svr_region_grow(vox.ctypes.data_as(C.c_void_p), 40, 4, 4, 0, xyz, 1, C.byref(p), C.c_void_p(mask), C.byref(st)) == code
            assert lib.svr_last_error_code() == code and b"svr_region_grow" in lib.svr_last_error()
            lib.svr_clear_error()
        p = dev.region_params(0, 100)
        for seeds, n in (((C.c_int32 * 3)(40, 0, 0), 1), (xyz, 0), (xyz, 65)):
            assert lib.svr_region_grow(vox.ctypes.data_as(C.c_void_p), 40, 4, 4, 0, seeds, n, C.byref(p), C.c_void_p(mask), C.byref(st)) == -3
            lib.svr_clear_error()
        assert lib.svr_region_apply(vox.ctypes.data_as(C.c_void_p), 40, 4, 4, 0, C.c_void_p(mask), 5, 0, C.c_void_p(mask)) == -3
        lib.svr_clear_error()
        with pytest.raises(host.SvrError):
            dev.region_grow(vox, [(0, 0, 9)], 0, 100)
        assert (dev.to_host(mask, (words,), np.uint32) == 0xABABABAB).all()
        # and a good call still works afterwards
        check(dev, "noise", vox, rr.spread_seeds(vox), rr.NOISE_LO, rr.NOISE_HI, 6)
    finally:
        dev.free(mask)
