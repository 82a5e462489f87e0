"""svr_set_option / svr_get_option against the answers recorded in tests/golden/option_answers.json (tests/golden/make_option_answers.py):
the default of every key before any set, and for every key and probe value the return code, the full text of svr_last_error() and the value
svr_get_option reports afterwards.  The two calls touch only the host context and the error record, so the library answers them without a
GPU.  Options persist in a process: the answers are taken in a fresh child process, in the order of the recording.  The recording keeps
a probe as [return code, svr_get_option afterwards, index of its text]; a text that holds the probed value as "bad value <v>" is kept once
per key with the value as {d} (decimal) or {x} (hexadecimal), and the test compares the text it rebuilds from that, character by character."""
import json
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = Path(__file__).resolve().parent / "golden" / "option_answers.json"
VALUES = [-2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 23, 32, 63, 64, 65, 128, 256, 257, 2**31 - 1]
LM_TUNE_VALUES = [0x01010101, 0x18010101, 0x00410101, 0x40404040]


def header_keys():
    """name -> key of every SVR_OPT_* of include/svr_abi.h, then the key without a name (101) and one no option has (9999)"""
    header = (ROOT / "include" / "svr_abi.h").read_text()
    keys = {name: int(key) for name, key in re.findall(r"^#define (SVR_OPT_\w+) (\d+)\b", header, flags=re.M)}
    keys["key 101"] = 101
    keys["unknown key 9999"] = 9999
    return keys


def answers():
    """what the library at hand answers, in this process (which must not have set an option before)"""
    from sunvolumerender_amd import abi

    lib = abi.load()
    lib.svr_set_error_mode(0)
    keys = header_keys()
    out = {"keys": keys, "defaults": {name: lib.svr_get_option(key) for name, key in keys.items()}, "probes": {}}
    for name, key in keys.items():
        probes = out["probes"][name] = {}
        for value in VALUES + (LM_TUNE_VALUES if name == "SVR_OPT_LM_TUNE" else []):
            lib.svr_clear_error()
            rc = lib.svr_set_option(key, value)
            assert lib.svr_last_error_code() == rc
            probes[str(value)] = [rc, lib.svr_last_error().decode(), lib.svr_get_option(key)]
    lib.svr_clear_error()
    return out


def answers_of_a_fresh_process():
    code = ("import sys, json; sys.path.insert(0, %r)\n"
            "from tests import test_options_cpu as t\n"
            "print('ANSWERS ' + json.dumps(t.answers()))\n") % str(ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("ANSWERS ")][-1][len("ANSWERS "):])


def test_every_option_of_the_header_is_recorded():
    assert header_keys() == json.loads(GOLDEN.read_text())["keys"], "the recording holds other keys: run tests/golden/make_option_answers.py"


def fill(template, value):
    return template.replace("{d}", str(value)).replace("{x}", "%x" % (value & 0xffffffff))


def pack(probes):
    """{value: [rc, text, get]} of one key -> {"texts": templates, "answers": [[rc, get] or [rc, get, template index]] in probe order}"""
    texts, answers = [], []
    for value, (rc, text, got) in probes.items():
        if text == "":
            answers.append([rc, got])
            continue
        for mark, shown in (("{d}", value), ("0x{x}", "0x%x" % (int(value) & 0xffffffff))):
            tpl = text.replace(f"bad value {shown}", f"bad value {mark}", 1)
            if tpl != text and fill(tpl, int(value)) == text:
                text = tpl
                break
        if text not in texts:
            texts.append(text)
        answers.append([rc, got, texts.index(text)])
    return {"texts": texts, "answers": answers}


def unpack(name, packed):
    values = VALUES + (LM_TUNE_VALUES if name == "SVR_OPT_LM_TUNE" else [])
    assert len(values) == len(packed["answers"]), name
    return {str(v): [a[0], fill(packed["texts"][a[2]], v) if len(a) > 2 else "", a[1]] for v, a in zip(values, packed["answers"])}


def test_options_match_the_recording():
    recorded = json.loads(GOLDEN.read_text())
    assert recorded["values"] == VALUES and recorded["lm_tune_values"] == LM_TUNE_VALUES
    got = answers_of_a_fresh_process()
    assert got["keys"] == recorded["keys"]
    assert got["defaults"] == recorded["defaults"]
    assert list(got["probes"]) == list(recorded["probes"])
    for name in recorded["keys"]:
        expected = unpack(name, recorded["probes"][name])
        for value, answer in expected.items():
            assert got["probes"][name][value] == answer, (name, value)
        assert got["probes"][name] == expected
