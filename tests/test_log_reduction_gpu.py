"""The integer range reduction of the device logarithms (svr_math.hpp: logf_unit, logf_) against the oracle's svo_logf, which keeps
the compare / select form: bit for bit, on the inputs where the two exponent / mantissa splits could part -- the mantissas around the
sqrt(2) threshold 0x3504f3 at every binary exponent -- and on what the Woodcock walk really passes, 1 - u of _curand_uniform's mapping.

One CPU-only check needs no device: which generator words make 1 - u exactly 0.
"""
import ctypes as C

import numpy as np
import pytest

FN_LOG, FN_LOG_UNIT = 1, 10
THRESHOLD = 0x3504F3            # mantissa bits of 1.41421356f: above it the reduction halves m and increments e


def _mantissas():
    return np.concatenate([np.array([0, 1, 0x7FFFFF], dtype=np.uint32), np.arange(THRESHOLD - 64, THRESHOLD + 65, dtype=np.uint32)])


def _at_exponents(lo, hi):
    """every mantissa of _mantissas() at the biased exponents lo .. hi"""
    e = np.arange(lo, hi + 1, dtype=np.uint32)
    return ((e[:, None] << np.uint32(23)) | _mantissas()[None, :]).ravel()


def uniform_of_words(words):
    """_curand_uniform as the device computes it: fma(float(word), 2^-32, 2^-33).  The product is exact (a power-of-two scaling),
    so one float32 add models the fma's single rounding."""
    return np.asarray(words, dtype=np.uint32).astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)


def _walk_arguments():
    words = np.random.default_rng(20250).integers(0, 2 ** 32, size=65536, dtype=np.uint64).astype(np.uint32)
    return (np.float32(1.0) - uniform_of_words(words)).view(np.uint32)


def unit_inputs():
    """bit patterns for logf_unit"""
    return np.concatenate([_at_exponents(1, 127), np.array([0], dtype=np.uint32), _walk_arguments()])


def log_inputs():
    """bit patterns for logf_: the same, the exponents above 1, subnormals and the special values"""
    special = np.array([1, 2, THRESHOLD, 0x7FFFFF,                                      # subnormals
                        0x00000000, 0x80000000, 0x7F800000, 0x7FC00000, 0xBF800000,     # +0, -0, +inf, NaN, -1
                        0x7F7FFFFF], dtype=np.uint32)                                   # FLT_MAX
    return np.concatenate([unit_inputs(), _at_exponents(128, 254), special])


_REF = {}


def _oracle_log(bits):
    """svo_logf of every input, as bits; computed once per input set"""
    key = bits.tobytes()
    if key not in _REF:
        from oracle import binding

        f = binding.load().svo_logf
        out = np.array([f(float(x)) for x in bits.view(np.float32)], dtype=np.float32).view(np.uint32)
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _device(dev, fn, bits):
    a = np.ascontiguousarray(bits.view(np.float32).reshape(-1, 1))
    out = np.zeros(a.shape[0], dtype=np.float32)
    dev.check(dev.lib.svr_selftest_math(fn, a.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p), a.shape[0]))
    return out.view(np.uint32)


def _assert_same_bits(got, want, x, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} differ; first x = {[hex(v) for v in x[bad[:3]]]}: "
                           f"got {[hex(v) for v in got[bad[:3]]]}, want {[hex(v) for v in want[bad[:3]]]}")


@pytest.mark.gpu
def test_logf_unit_matches_the_oracle_bit_for_bit(hip_dev):
    x = unit_inputs()
    assert x.size == 127 * 132 + 1 + 65536
    _assert_same_bits(_device(hip_dev, FN_LOG_UNIT, x), _oracle_log(x), x, "logf_unit vs svo_logf")


@pytest.mark.gpu
def test_logf_matches_the_oracle_bit_for_bit(hip_dev):
    x = log_inputs()
    assert x.size == 254 * 132 + 1 + 65536 + 10
    _assert_same_bits(_device(hip_dev, FN_LOG, x), _oracle_log(x), x, "logf_ vs svo_logf")


def test_one_minus_uniform_is_zero_exactly_from_word_ffffff80():
    """1 - u == 0 (the walk's log(0) = -inf) exactly for the words >= 0xFFFFFF80: their float conversion rounds to 2^32, u to 1;
    0xFFFFFF7F converts to 0xFFFFFF00 and gives u = 1 - 2^-24."""
    words = np.arange(0xFFFFFF00, 0x100000000, dtype=np.uint64).astype(np.uint32)
    zero = (np.float32(1.0) - uniform_of_words(words)) == np.float32(0.0)
    assert np.array_equal(zero, words >= np.uint32(0xFFFFFF80))
    assert uniform_of_words([0xFFFFFF7F])[0] == np.float32(1.0 - 2.0 ** -24)
