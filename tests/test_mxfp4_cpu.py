"""MXFP4 without a GPU: the numpy restatement of the quantisation rule (tests/mxfp4_ref.py) has the properties
include/sli.h states, and the host-only parts of the interface (sli_mxfp4_bytes, the dtype name) are in place."""
import ctypes

import numpy as np
import pytest

from tests import mxfp4_ref as mx


def _block(vals, fill=0.0):
    b = np.full((1, 32), fill, np.float32)
    b[0, :len(vals)] = vals
    return b


def test_all_codes_decode_per_table():
    codes = np.tile(np.arange(16, dtype=np.uint8), 2)[None, :]
    want = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0.0, -.5, -1, -1.5, -2, -3, -4, -6], np.float32)
    for byte, f in ((127, 1.0), (128, 2.0), (120, 2.0 ** -7), (0, 2.0 ** -127), (252, 2.0 ** 125)):
        got = mx.dequantize(codes, np.array([[byte]], np.uint8))[0, :16]
        exp = (want.astype(np.float64) * f).astype(np.float32)
        assert np.array_equal(got, exp), byte
        assert np.array_equal(np.signbit(got), np.signbit(want))


def test_ties_go_to_the_even_code():
    # amax = 6 gives e = 0, so the values are their own scaled magnitudes
    c, s = mx.quantize(_block([6.0, .25, .75, 1.25, 1.75, 2.5, 3.5, 5.0, -.25, -.75, -1.25, -1.75, -2.5, -3.5, -5.0]))
    assert s[0, 0] == 127
    assert list(c[0, :15]) == [7, 0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14]
    for tie, lo in zip(mx.TIES, range(7)):
        below = np.nextafter(tie, np.float32(0))
        above = np.nextafter(tie, np.float32(8))
        c, _ = mx.quantize(_block([6.0, below, above]))
        assert list(c[0, 1:3]) == [lo, lo + 1]


def test_values_above_six_saturate():
    c, s = mx.quantize(_block([7.9, 6.5, -7.0, 5.5, 5.0, 6.0]))
    assert s[0, 0] == 127  # floor(log2(7.9)) - 2 = 0
    assert list(c[0, :6]) == [7, 7, 15, 7, 6, 7]


def test_zero_block_and_scale_range():
    c, s = mx.quantize(np.zeros((2, 64), np.float32))
    assert np.all(s == 127) and np.all(c == 0)
    c, s = mx.quantize(_block([np.float32(1e-45)]))  # the smallest denormal: e clamps at -127
    assert s[0, 0] == 0 and c[0, 0] == 0
    c, s = mx.quantize(_block([np.finfo(np.float32).max]))
    assert s[0, 0] == 127 + 125 and c[0, 0] == 7  # 2^127 (2 - 2^-23) / 2^125 > 5
    # exactly at / just under a power of two
    c, s = mx.quantize(_block([4.0]))
    assert s[0, 0] == 127 and c[0, 0] == 6
    c, s = mx.quantize(_block([np.nextafter(np.float32(4.0), np.float32(0))]))
    assert s[0, 0] == 126 and c[0, 0] == 7


def test_requantising_a_dequantised_tensor_is_the_identity():
    w = mx.crafted(6, 256, seed=3)
    c, s = mx.quantize(w)
    d = mx.dequantize(c, s)
    c2, s2 = mx.quantize(d)
    d2 = mx.dequantize(c2, s2)
    assert np.array_equal(d, d2)
    assert np.array_equal(np.signbit(d), np.signbit(d2))
    # where a block kept its largest code at 4 or 6 the scale and codes are reproduced too
    keep = (c.reshape(6, 8, 32) & 7).max(axis=2) >= 6
    assert np.array_equal(s[keep], s2[keep])


def test_pack_order():
    codes = np.arange(64, dtype=np.uint8).reshape(2, 32) & 15
    codes[1] = codes[1][::-1]
    d = mx.pack(codes)
    assert d.shape == (2, 16) and d.dtype == np.uint8
    assert d[0, 0] == (0 | (1 << 4)) and d[0, 3] == (6 | (7 << 4))
    assert d[1, 0] == (15 | (14 << 4))
    assert np.array_equal(mx.unpack(d), codes)


def test_same_codes_ignores_only_the_sign_of_zero():
    assert mx.same_codes(np.array([0, 8, 3]), np.array([8, 0, 3]))
    assert not mx.same_codes(np.array([1]), np.array([9]))


def test_mxfp4_bytes_host_only():
    from simplellminference_amd import _lib
    L = _lib.load()
    d, s = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.sli_mxfp4_bytes(1, 32, ctypes.byref(d), ctypes.byref(s)) == 0
    assert (d.value, s.value) == (16, 1)
    assert L.sli_mxfp4_bytes(3, 11008, ctypes.byref(d), ctypes.byref(s)) == 0
    assert (d.value, s.value) == (3 * 5504, 3 * 344)
    assert L.sli_mxfp4_bytes(5, 48, ctypes.byref(d), ctypes.byref(s)) == 2  # SLI_ERR_SHAPE


def test_dtype_names():
    from simplellminference_amd import _lib, model
    assert _lib.DT_MXFP4 == 3
    assert model._DTYPES["mxfp4"] == 3 and model._DTYPES["fp4"] == 3
