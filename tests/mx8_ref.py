"""MXFP8 activations in numpy: the quantisation rule that include/sli.h documents (sli_quant_mxfp8) and the device
quantisers must reproduce bit for bit, on tests/kv8_ref.py's E4M3 codec (written from the format alone).

An [M, K] image (K % 32 == 0): codes uint8 [M, K] (E4M3), scales uint8 [M, K/32] (e8m0, value 2^(byte - 127)).
"""
import numpy as np

from tests import kv8_ref as f8

BLOCK = 32
EMAX = 8  # 448 = 1.75 * 2^8


def quantize(v):
    """fp32 [M, K] -> (codes, scale bytes). e = clamp(floor(log2(amax)) - 8, -127, 127), amax == 0: e = 0."""
    v = np.ascontiguousarray(v, np.float32)
    M, K = v.shape
    assert K % BLOCK == 0
    b = v.reshape(M, K // BLOCK, BLOCK)
    amax = np.abs(b).max(axis=2)
    _, ex = np.frexp(amax)  # floor(log2(amax)) = ex - 1, exact (denormals too)
    e = np.where(amax == 0, 0, np.clip(ex.astype(np.int32) - 1 - EMAX, -127, 127)).astype(np.int32)
    s = np.ldexp(b.astype(np.float64), -e[:, :, None])  # exact
    return f8.encode(s).reshape(M, K), (e + 127).astype(np.uint8)


def dequantize(codes, scales):
    """-> float64 [M, K], exact."""
    M, K = codes.shape
    val = f8.TABLE64[np.asarray(codes, np.uint8)].reshape(M, K // BLOCK, BLOCK)
    return np.ldexp(val, scales.astype(np.int32)[:, :, None] - 127).reshape(M, K)

