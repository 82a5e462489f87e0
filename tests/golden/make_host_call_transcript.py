#!/usr/bin/env python3
"""tests/golden/host_call_transcript.json: the library calls that the volume-op methods of host.Device make for the rows of ROWS, as the
fake device of tests/host_fake.py hears them -- per row the svr_* functions in order with every argument (scalars, struct members, buffer
sizes and the SHA-1 of buffer contents, no addresses) and the rendered return value.  Recorded from the commit BEFORE the methods were
rewritten on the staging scope of volume_ops.py; tests/test_host_staging_cpu.py replays it.  Run it again only when a call is meant to
change:  python tests/golden/make_host_call_transcript.py"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from sunvolumerender_amd import abi, host  # noqa: E402
from tests.host_fake import Dev, Lib, Out, run_row  # noqa: E402

GOLDEN = Path(__file__).with_name("host_call_transcript.json")

# Three distinct dimensions, so that a swapped axis shows; nx = 33 gives two mask words per row, 31 padding bits in the second.
S = (2, 3, 33)
N, W = 2 * 3 * 33, host.region_mask_words(S)
G = (3, 2, 5)                                                                # the resample rows' output shape (nz, ny, nx)
GRID = ((0, 33 * 65536 // 5, 5), (0, 3 * 65536 // 2, 2), (0, 2 * 65536 // 3, 3))
SUB, OFFSET = (1, 2, 5), (7, 1, 0)                                           # the paste rows' sub-mask and its offset (x, y, z)
BOX = ((1, 0, 0), (30, 2, 1))

_rng = np.random.default_rng(20240607)
VOL = _rng.integers(0, 65536, S).astype(np.uint16)
M, M2 = _rng.random(S) < 0.5, _rng.random(S) < 0.3
LAB = _rng.integers(0, 4, S).astype(np.uint32)                               # labels 0 .. 3: count = 3
D2 = _rng.integers(0, 100, S).astype(np.uint32)
KEEP = np.array([0, 1, 0, 1], dtype=np.uint8)
TABLE = np.zeros(3, dtype=host.COMPONENT_DTYPE)
TABLE["voxels"], TABLE["first"] = (60, 50, 40), (0, 1, 2)
SEEDS = np.array([[1, 1, 0], [32, 2, 1]], dtype=np.int32)
CLASSES = np.array([2, 5], dtype=np.uint32)
SUBMASK = _rng.random(SUB) < 0.5
VERTS = _rng.integers(0, 2048, (4, 3)).astype(np.int32)
TRIS = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
COUNTS = _rng.integers(0, 9, 64).astype(np.uint32)
PALETTE = np.array([[255, 0, 0, 255], [0, 255, 0, 128]], dtype=np.uint8)
VOLUME = host.create_device_volume(5, (33, 3, 2), (1.0, 1.0, 2.0), 4095.0)
SLICE = abi.SliceParams()


def R(rid, name, *args, **kwargs):
    return (rid, name, args, kwargs)


# (id, method of Device or "host.NAME", args, kwargs).  Dev(array): the array in a device buffer of the caller; Out(nbytes): a device
# buffer of the caller for the result; Lib: the library.  A "/host" row passes arrays, its "/dev" twin pointers with shape= and out_ptr=.
ROWS = [
    R("region_grow/host", "region_grow", VOL, SEEDS, 100, 60000, connectivity=26, box=BOX, max_sweeps=5),
    R("region_grow/dev", "region_grow", Dev(VOL), SEEDS, 100, 60000, shape=S, mask_ptr=Out(4 * W)),
    R("region_stats_of/host", "region_stats_of", VOL, M),
    R("region_stats_of/dev", "region_stats_of", Dev(VOL), Dev(M), shape=S),
    R("region_apply/host", "region_apply", VOL, M, abi.REGION_REMOVE, 7),
    R("region_apply/dev", "region_apply", Dev(VOL), Dev(M), shape=S, out_ptr=Out(2 * N)),
    R("region_morph/host", "region_morph", M, abi.MORPH_OPEN, 18, 2),
    R("region_morph/dev", "region_morph", Dev(M), abi.MORPH_DILATE, shape=S, out_ptr=Out(4 * W)),
    R("region_combine/host", "region_combine", M, M2, abi.MASK_ANDNOT),
    R("region_combine/not", "region_combine", M, None, abi.MASK_NOT),
    R("region_combine/dev", "region_combine", Dev(M), Dev(M2), abi.MASK_OR, shape=S, out_ptr=Out(4 * W)),
    R("region_reconstruct/host", "region_reconstruct", M, M2, 18, 3),
    R("region_reconstruct/dev", "region_reconstruct", Dev(M), Dev(M2), shape=S, out_ptr=Out(4 * W)),
    R("region_fill_holes/host", "region_fill_holes", M, 26, 4),
    R("region_fill_holes/dev", "region_fill_holes", Dev(M), shape=S, out_ptr=Out(4 * W)),
    R("region_detach/host", "region_detach", M, SEEDS, 18, 2, 26, 9),
    R("region_detach/dev", "region_detach", Dev(M), SEEDS, shape=S, out_ptr=Out(4 * W)),
    R("region_threshold/host", "region_threshold", VOL, 10, 2000, BOX),
    R("region_threshold/dev", "region_threshold", Dev(VOL), 10, 2000, shape=S, out_ptr=Out(4 * W)),
    R("region_label/host", "region_label", M, 18),
    R("region_label/dev", "region_label", Dev(M), shape=S, out_ptr=Out(4 * N)),
    R("region_label_table/host", "region_label_table", LAB, 3),
    R("region_label_table/host_vox", "region_label_table", LAB, 3, VOL),
    R("region_label_table/dev", "region_label_table", Dev(LAB), 3, Dev(VOL), shape=S, out_ptr=Out(120)),
    R("region_select/host", "region_select", LAB, 3, KEEP),
    R("region_select/dev", "region_select", Dev(LAB), 3, KEEP, shape=S, out_ptr=Out(4 * W)),
    R("region_select_by_size/host", "region_select_by_size", LAB, 3),
    R("region_select_by_size/host_table", "region_select_by_size", LAB, 3, TABLE, 2, 1),
    R("region_select_by_size/dev", "region_select_by_size", Dev(LAB), 3, Dev(TABLE), shape=S, out_ptr=Out(4 * W)),
    R("region_distance/host", "region_distance", M, weights=(1, 2, 3), target=abi.DIST_TO_UNSET),
    R("region_distance/dev", "region_distance", Dev(M), shape=S, out_ptr=Out(4 * N)),
    R("region_distance_select/host", "region_distance_select", D2, 1, 50),
    R("region_distance_select/dev", "region_distance_select", Dev(D2), 1, 50, shape=S, out_ptr=Out(4 * W)),
    R("region_ball/host", "region_ball", M, abi.MORPH_CLOSE, 9, (1, 1, 4)),
    R("region_ball/dev", "region_ball", Dev(M), abi.MORPH_ERODE, 4, shape=S, out_ptr=Out(4 * W)),
    R("region_distance_max/host", "region_distance_max", D2),
    R("region_distance_max/host_mask", "region_distance_max", D2, M),
    R("region_distance_max/dev", "region_distance_max", Dev(D2), Dev(M), shape=S),
    R("region_distance_volume/host", "region_distance_volume", D2, 3),
    R("region_distance_volume/dev", "region_distance_volume", Dev(D2), shape=S, out_ptr=Out(2 * N)),
    R("region_geodesic/host", "region_geodesic", LAB, M),
    R("region_geodesic/host_zones", "region_geodesic", LAB, M, step_weights=(3, 3, 3, 4, 4, 4, 5), max_sweeps=7, want_dist=False),
    R("region_geodesic/mixed", "region_geodesic", Dev(LAB), M, want_zones=False),
    R("region_geodesic/dev", "region_geodesic", Dev(LAB), Dev(M), shape=S, dist_ptr=Out(4 * N), zones_ptr=Out(4 * N)),
    R("region_seed_labels/host", "region_seed_labels", SEEDS, S),
    R("region_seed_labels/dev", "region_seed_labels", SEEDS, S, out_ptr=Out(4 * N)),
    R("region_split/host", "region_split", M, 4, 18, (1, 1, 2), None, 6),
    R("region_split/dev", "region_split", Dev(M), 4, step_weights=(1, 1, 1, 0, 0, 0, 0), shape=S, out_ptr=Out(4 * N)),
    R("region_zone_cut/host", "region_zone_cut", LAB, 6),
    R("region_zone_cut/dev", "region_zone_cut", Dev(LAB), shape=S, out_ptr=Out(4 * W)),
    R("region_growcut/host", "region_growcut", VOL, LAB),
    R("region_growcut/host_domain", "region_growcut", VOL, LAB, M, connectivity=6, gain=2, shift=1, max_sweeps=8, want_cost=False),
    R("region_growcut/dev", "region_growcut", Dev(VOL), Dev(LAB), Dev(M), shape=S, step_weights=(1, 1, 2, 0, 0, 0, 0), cost_ptr=Out(4 * N),
      zones_ptr=Out(4 * N)),
    R("region_seed_classes/host", "region_seed_classes", SEEDS, CLASSES, S),
    R("region_seed_classes/dev", "region_seed_classes", SEEDS, CLASSES, S, out_ptr=Out(4 * N)),
    R("region_label_paint/host", "region_label_paint", LAB, M, 9, True),
    R("region_label_paint/dev", "region_label_paint", Dev(LAB), Dev(M), 9, shape=S),
    R("volume_histogram/host", "volume_histogram", VOL),
    R("volume_histogram/host_mask", "volume_histogram", VOL, M, 100, 1123, 2, BOX),
    R("volume_histogram/dev", "volume_histogram", Dev(VOL), Dev(M), 0, 255, shape=S, out_ptr=Out(4 * 256)),
    R("region_label_histogram/host", "region_label_histogram", LAB, VOL, 3, 0, 1023, 4),
    R("region_label_histogram/refused", "region_label_histogram", LAB, VOL, 3, 5, 4),
    R("region_label_histogram/dev", "region_label_histogram", Dev(LAB), Dev(VOL), 3, 0, 63, shape=S, out_ptr=Out(4 * 4 * 64)),
    R("mesh_isosurface/host", "mesh_isosurface", VOL, 500, 2),
    R("mesh_isosurface/dev", "mesh_isosurface", Dev(VOL), 500, shape=S),
    R("mesh_region/host", "mesh_region", M, 1),
    R("mesh_region/dev", "mesh_region", Dev(M), shape=S),
    R("mesh_measure/host", "mesh_measure", VERTS, TRIS),
    R("mesh_measure/empty", "mesh_measure", np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), (0.5, 0.5, 1.0)),
    R("volume_rank/host", "volume_rank", VOL, abi.FILTER_MAX, 18, 2),
    R("volume_rank/dev", "volume_rank", Dev(VOL), abi.FILTER_MIN, shape=S, out_ptr=Out(2 * N)),
    R("volume_median/host", "volume_median", VOL, 26, 3),
    R("volume_median/dev", "volume_median", Dev(VOL), shape=S, out_ptr=Out(2 * N)),
    R("volume_smooth/host", "volume_smooth", VOL, (1, 0, 2)),
    R("volume_smooth/dev", "volume_smooth", Dev(VOL), (2, 2, 2), shape=S, out_ptr=Out(2 * N)),
    R("volume_resample/host", "volume_resample", VOL, GRID, abi.RESAMPLE_LINEAR),
    R("volume_resample/dev", "volume_resample", Dev(VOL), GRID, shape=S, out_ptr=Out(2 * 30)),
    R("volume_crop/host", "volume_crop", VOL, BOX),
    R("volume_crop/dev", "volume_crop", Dev(VOL), BOX, shape=S, out_ptr=Out(2 * N)),
    R("region_resample/host", "region_resample", M, GRID),
    R("region_resample/dev", "region_resample", Dev(M), GRID, shape=S, out_ptr=Out(4 * host.region_mask_words(G))),
    R("region_label_resample/host", "region_label_resample", LAB, GRID),
    R("region_label_resample/dev", "region_label_resample", Dev(LAB), GRID, shape=S, out_ptr=Out(4 * 30)),
    R("region_paste/host", "region_paste", SUBMASK, M, OFFSET),
    R("region_paste/host_or", "region_paste", SUBMASK, M, OFFSET, abi.MASK_OR),
    R("region_paste/mixed", "region_paste", SUBMASK, Dev(M), OFFSET, full_shape=S),
    R("region_paste/dev", "region_paste", Dev(SUBMASK), Dev(M), OFFSET, sub_shape=SUB, full_shape=S),
    R("region_mask_expand/host", "region_mask_expand", M, 255),
    R("region_mask_expand/dev", "region_mask_expand", Dev(M), shape=S, out_ptr=Out(N)),
    R("region_measure", "region_measure", abi.RegionStats(), (0.5, 1.0, 2.0)),
    # parameters, timers, overlays and the Device forms of the host-only helpers: they stage nothing
    R("region_params", "region_params", 5, 9, 18, BOX, 3),
    R("growcut_params", "growcut_params", (1, 2, 3, 4, 5, 6, 7), 18, 2, 1, 4),
    R("histogram_params", "histogram_params", 1, 9, 1, BOX),
    R("mesh_params", "mesh_params", 7, 2),
    R("region_label_last_ms", "region_label_last_ms"),
    R("region_distance_last_ms", "region_distance_last_ms"),
    R("region_distance_pass_ms", "region_distance_pass_ms"),
    R("region_geodesic_last_ms", "region_geodesic_last_ms"),
    R("region_growcut_last_ms", "region_growcut_last_ms"),
    R("volume_histogram_last_ms", "volume_histogram_last_ms"),
    R("overlay_last_ms", "overlay_last_ms"),
    R("mesh_last_ms", "mesh_last_ms"),
    R("volume_filter_last_ms", "volume_filter_last_ms"),
    R("volume_resample_last_ms", "volume_resample_last_ms"),
    R("overlay_style", "overlay_style", 10, 20, PALETTE),
    R("overlay_palette_default", "overlay_palette_default", 4),
    R("slice_ids", "slice_ids", Out(4 * 64), VOLUME, S, 8, 8, SLICE, mask=Dev(M), count=1, spacing=0.5),
    R("hit_ids", "hit_ids", Out(4 * 64), Out(40 * 64), 8, 8, VOLUME, S, labels=Dev(LAB)),
    R("overlay_ids", "overlay_ids", Out(4 * 64), Out(4 * 64), 8, 8),
    R("overlay_slice", "overlay_slice", Out(4 * 64), VOLUME, S, 8, 8, SLICE, labels=Dev(LAB)),
    R("resample_grid_box", "resample_grid_box", S, BOX),
    R("resample_grid_spacing", "resample_grid_spacing", S, (1.0, 1.0, 2.0), 0.5),
    R("resample_grid_dims", "resample_grid_dims", S, G, BOX),
    R("resample_grid_place", "resample_grid_place", VOLUME, S, GRID),
    R("mesh_positions", "mesh_positions", VERTS, (1.0, 2.0, 3.0), VOLUME),
    # the module-level helpers on the library's host code
    R("host.mesh_positions", "host.mesh_positions", Lib, VERTS, (1.0, 2.0, 3.0)),
    R("host.distance_weights", "host.distance_weights", (1.0, 1.0, 2.0), S, Lib),
    R("host.geodesic_weights", "host.geodesic_weights", (1.0, 1.0, 2.0), 18, S, Lib),
    R("host.smooth_radii", "host.smooth_radii", (1.0, 1.0, 2.0), 1.5, Lib),
    R("host.histogram_bins", "host.histogram_bins", 0, 255, 2, Lib),
    R("host.histogram_bin_range", "host.histogram_bin_range", 3, 0, 255, 2, Lib),
    R("host.histogram_moments", "host.histogram_moments", COUNTS, Lib),
    R("host.histogram_quantile", "host.histogram_quantile", COUNTS, 1, 2, Lib),
    R("host.histogram_otsu", "host.histogram_otsu", COUNTS, 3, Lib),
    R("host.region_seed_from_world", "host.region_seed_from_world", Lib, VOLUME, (33, 3, 2), (0.25, -0.5, 1.0)),
]


def record(row):
    """{"calls": the transcript, "result": the rendered return value} of one row on a fresh fake device."""
    dev, _, result = run_row(row)
    if isinstance(result, Exception):
        raise result
    return {"calls": dev.lib.calls, "result": dev.render(result)}


def main():
    out = {row[0]: record(row) for row in ROWS}
    GOLDEN.write_text("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(sum(len(v["calls"]) for v in out.values()), "calls of", len(out), "rows,", GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
