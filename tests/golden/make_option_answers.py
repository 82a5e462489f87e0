#!/usr/bin/env python3
"""tests/golden/option_answers.json: what the library at hand answers to the calls of tests/test_options_cpu.py -- the default of every
option key, and [return value, text of svr_last_error(), svr_get_option afterwards] per key and probe value.  Recorded from the PARENT's
library, the commit BEFORE the C-ABI host file was split into one translation unit per concern (its id stands in the file); run it
again only when an option is added or an answer is meant to change:  python tests/golden/make_option_answers.py [parent commit id]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests import test_options_cpu as t  # noqa: E402


def main():
    old = json.loads(t.GOLDEN.read_text()) if t.GOLDEN.exists() else {}
    out = {"recorded_from_commit": sys.argv[1] if len(sys.argv) > 1 else old.get("recorded_from_commit", "unknown")}
    out.update(t.answers_of_a_fresh_process())
    out["values"], out["lm_tune_values"] = t.VALUES, t.LM_TUNE_VALUES
    packed = {name: t.pack(p) for name, p in out["probes"].items()}
    assert all(t.unpack(name, packed[name]) == out["probes"][name] for name in packed)
    # one line per key
    rows = [f' {json.dumps(k)}: {json.dumps(out[k])}' for k in ("recorded_from_commit", "values", "lm_tune_values", "keys", "defaults")]
    rows.append(' "probes": {\n' + ",\n".join(f"  {json.dumps(name)}: {json.dumps(p)}" for name, p in packed.items()) + "\n }")
    t.GOLDEN.write_text("{\n" + ",\n".join(rows) + "\n}\n")
    print(sum(len(p) for p in out["probes"].values()), "probes of", len(out["keys"]), "keys")


if __name__ == "__main__":
    main()
