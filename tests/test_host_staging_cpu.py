"""The Python host layer of the volume operations on the fake device of tests/host_fake.py (no library, no GPU): every row of
tests/golden/make_host_call_transcript.py makes exactly the library calls recorded in tests/golden/host_call_transcript.json before the
methods were rewritten on the staging scope, and leaves no device memory behind, however the call ends."""
import json

import numpy as np
import pytest

from sunvolumerender_amd import host
from sunvolumerender_amd.host import SvrError
from tests.golden.make_host_call_transcript import CLASSES, GOLDEN, KEEP, LAB, M, M2, ROWS, S, SEEDS, VOL, R, record
from tests.host_fake import FAKE_BASE, run_row

RECORDED = json.loads(GOLDEN.read_text())
IDS = [row[0] for row in ROWS]


def test_every_row_is_recorded():
    assert list(RECORDED) == IDS


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_replay(row):
    assert json.loads(json.dumps(record(row))) == RECORDED[row[0]]


def _pointers(result):
    if isinstance(result, tuple):
        return [p for r in result for p in _pointers(r)]
    return [result] if isinstance(result, int) and not isinstance(result, bool) and result >= FAKE_BASE else []


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_no_leak_on_success(row):
    dev, caller, result = run_row(row)
    assert not isinstance(result, Exception)
    assert dev.live == set(caller)                            # the caller's buffers, untouched by free, and nothing else
    returned = _pointers(result)
    assert set(returned) <= set(caller)
    if returned:                                              # a result left on the device is complete when the method returns
        assert dev.lib.syncs >= 1 and dev.lib.last_sync_at == len(dev.lib.calls)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_no_leak_on_failure(row):
    dev, caller, _ = run_row(row)
    mallocs, calls = dev.nmalloc, dev.lib.ncalls
    for k in range(1, mallocs + 1):
        dev, caller, result = run_row(row, fail_malloc=k)
        assert isinstance(result, SvrError) and "injected malloc failure" in str(result), (k, result)
        assert dev.live == set(caller), f"malloc {k} of {mallocs} failed"
    for k in range(1, calls + 1):
        dev, caller, result = run_row(row, fail_call=k)
        assert isinstance(result, SvrError) and "injected failure of svr_" in str(result), (k, result)
        assert dev.live == set(caller), f"library call {k} of {calls} failed"


T = (3, 2, 33)                                                # as many voxels as S, another shape
BAD_ARGUMENTS = [
    (R("region_select/keep", "region_select", LAB, 3, KEEP[:3]), "keep must have count \\+ 1 entries"),
    (R("region_growcut/shape", "region_growcut", VOL, LAB.reshape(T)), "the volume and the labels differ in shape"),
    (R("region_growcut/domain", "region_growcut", VOL, LAB, M[:1]), "reshape"),
    (R("region_label_table/shape", "region_label_table", LAB, 3, VOL.reshape(T)), "the volume and the labels differ in shape"),
    (R("region_label_histogram/shape", "region_label_histogram", LAB, VOL.reshape(T), 3), "the volume and the labels differ in shape"),
    (R("region_combine/shape", "region_combine", M, M2[:1], 1), "reshape"),
    (R("region_seed_classes/count", "region_seed_classes", SEEDS, CLASSES[:1], S), "one class per seed"),
]


@pytest.mark.parametrize("row,message", BAD_ARGUMENTS, ids=[row[0] for row, _ in BAD_ARGUMENTS])
def test_no_leak_on_argument_error(row, message):
    dev, caller, result = run_row(row)
    assert isinstance(result, ValueError), result
    with pytest.raises(ValueError, match=message):
        raise result
    assert dev.live == set(caller)


@pytest.mark.parametrize("call,message", [
    (lambda d: d.region_label(1, 6), "a device mask needs shape=\\(nz, ny, nx\\)"),
    (lambda d: d.region_apply(1, M), "a device volume needs shape=\\(nz, ny, nx\\)"),
    (lambda d: d.region_select(1, 3, KEEP), "device labels need shape=\\(nz, ny, nx\\)"),
    (lambda d: d.region_apply(VOL[0], M), "the volume must be \\[nz\\]\\[ny\\]\\[nx\\]"),
    (lambda d: d.region_zone_cut(LAB[0]), "the labels must be \\[nz\\]\\[ny\\]\\[nx\\]"),
    (lambda d: d.region_morph(M[0], 1), "a mask must be \\[nz\\]\\[ny\\]\\[nx\\]"),
])
def test_shape_rules(call, message):
    from tests.host_fake import FakeDevice
    dev = FakeDevice()
    with pytest.raises(ValueError, match=message):
        call(dev)
    assert not dev.live and not dev.lib.calls


def test_free_failure_does_not_replace_the_error():
    """A free that fails while the scope unwinds an exception leaves that exception in place; the other buffers are still freed."""
    from tests.host_fake import FakeDevice
    dev = FakeDevice()
    real_free, failed = dev.free, []

    def free(ptr):
        real_free(ptr)
        if not failed:
            failed.append(ptr)
            raise SvrError("free failed")
    dev.free = free
    dev.lib.fail_call = 1
    with pytest.raises(SvrError, match="injected failure of svr_region_combine"):
        dev.region_combine(M, M2, 1)
    assert failed and not dev.live


def test_mask_round_trip():
    words = host.region_mask_pack(M)
    assert words.dtype == np.uint32 and words.shape == (host.region_mask_words(S),) == (12,)
    assert np.array_equal(host.region_mask_unpack(words, S), M)
    assert not np.any(words.reshape(2, 3, 2)[:, :, 1] >> 1)   # nx = 33: bit 0 of the second word is voxel 32, the other 31 are padding
    assert np.array_equal(host.region_mask_unpack(host.region_mask_pack(np.ones(S, bool)), S), np.ones(S, bool))
    assert np.all(host.region_mask_pack(np.ones(S, bool)).reshape(2, 3, 2) == [0xFFFFFFFF, 1])
