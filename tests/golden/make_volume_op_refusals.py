#!/usr/bin/env python3
"""tests/golden/volume_op_refusals.json: what the library at hand answers to the calls of tests/test_volume_ops_refusals_cpu.py --
[return value, text of svr_last_error()] per entry point and case.  Recorded from the commit BEFORE the volume ops got their shared
host layer; run it again only when a refusal is meant to change:  python tests/golden/make_volume_op_refusals.py"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from sunvolumerender_amd import abi  # noqa: E402
from tests import test_volume_ops_refusals_cpu as t  # noqa: E402

# The arguments of every entry point that takes nx, ny, nz, in the order of include/svr_abi.h.  "x" "y" "z": the dimensions; "p": a
# zeroed buffer (seed (0, 0, 0), box 0 .. 0); "ones": uint32 ones (weights, radii); "spacing": doubles 1.0; "params": the defaults of
# svr_region_params_default; ["c", noun]: a connectivity / element argument, 6 unless it is the one under test; an int: itself.
CALLS = {
    "svr_region_mask_words": ["x", "y", "z"],
    "svr_region_default_max_sweeps": ["x", "y", "z"],
    "svr_region_grow": ["p", "x", "y", "z", 0, "p", 1, "params", "p", "p"],
    "svr_region_stats_of": ["p", "x", "y", "z", 0, "p", "p"],
    "svr_region_apply": ["p", "x", "y", "z", 0, "p", 1, 0, "p"],
    "svr_region_seed_from_world": ["p", "x", "y", "z", "p", "p"],
    "svr_region_morph": ["p", "x", "y", "z", 1, ["c", "element"], 1, "p"],
    "svr_region_combine": ["p", "p", "x", "y", "z", 1, "p"],
    "svr_region_reconstruct": ["p", "p", "x", "y", "z", ["c", "connectivity"], 0, "p", "p"],
    "svr_region_fill_holes": ["p", "x", "y", "z", ["c", "background connectivity"], 0, "p"],
    "svr_region_detach": ["p", "x", "y", "z", "p", 1, ["c", "element"], 1, ["c", "connectivity"], 0, "p", "p"],
    "svr_region_threshold": ["p", "x", "y", "z", 0, 0, 1, "p", "p", "p"],
    "svr_region_label": ["p", "x", "y", "z", ["c", "connectivity"], "p", "p"],
    "svr_region_label_table": ["p", "p", "x", "y", "z", 0, 1, "p"],
    "svr_region_select": ["p", "x", "y", "z", 1, "p", "p"],
    "svr_region_select_by_size": ["p", "x", "y", "z", 1, "p", 0, 0, "p", "p"],
    "svr_region_distance": ["p", "x", "y", "z", "ones", 1, "p"],
    "svr_region_distance_select": ["p", "x", "y", "z", 0, 1, "p"],
    "svr_region_ball": ["p", "x", "y", "z", 1, "ones", 1, "p"],
    "svr_region_distance_max": ["p", "p", "x", "y", "z", "p", "p", "p"],
    "svr_region_distance_volume": ["p", "x", "y", "z", 1, "p"],
    "svr_region_distance_weights": ["spacing", "x", "y", "z", "p", "p"],
    "svr_volume_rank": ["p", "x", "y", "z", 0, 1, ["c", "element"], 1, "p"],
    "svr_volume_smooth": ["p", "x", "y", "z", 0, "ones", "p"],
    "svr_region_geodesic_default_max_sweeps": ["x", "y", "z"],
    "svr_region_geodesic": ["p", "p", "x", "y", "z", "ones", 0, "p", "p", "p"],
    "svr_region_seed_labels": ["p", 1, "x", "y", "z", "p"],
    "svr_region_geodesic_weights": ["spacing", ["c", "connectivity"], "x", "y", "z", "p", "p"],
    "svr_region_split": ["p", "x", "y", "z", "ones", 1, ["c", "connectivity"], "ones", 0, "p", "p", "p", "p"],
    "svr_region_zone_cut": ["p", "x", "y", "z", ["c", "connectivity"], "p"],
}


def main():
    lib = abi.load()
    lib.svr_set_error_mode(0)
    out = {name: {"args": spec, "answers": {case: list(t.refusal(lib, name, spec, dims, noun)) for case, dims, noun in t.cases(spec)}}
           for name, spec in CALLS.items()}
    t.GOLDEN.write_text(json.dumps(out, indent=1) + "\n")
    print(sum(len(v["answers"]) for v in out.values()), "answers of", len(out), "entry points")


if __name__ == "__main__":
    main()
