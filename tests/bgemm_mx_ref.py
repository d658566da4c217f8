"""Inputs and float64 references for the batched decode projection from MXFP4 weights (bgemm.h bgemm_kernel<..,
mxfp4>, sli_batch_gemm_mxfp4), beside tests/bgemm_ref.py, whose launch restatement, epilogues and bounds apply as they
are once the weights are written as their dequantised values: a launch computes

  Y[b][r] = sum_kb 2^(s[r][kb] - 127) * sum_{k in block kb} code(W[r][k]) * (hi + lo)[b][k]

with no row scale; the cases below are bgemm_ref "case" dicts (W: the dequantised float64 matrix, scale: None) with
the codes, the packed data and the scale bytes beside them. The numpy rule of the format is tests/mxfp4_ref.py.
"""
from __future__ import annotations

import numpy as np

from tests import bgemm_ref as R
from tests import mxfp4_ref as mx

GRAIN = 2.0 ** -3            # 0.5 (the smallest non-zero code) * 2^-2 (scale byte 125) * 1 (an integer activation)
SCALE_BYTES = (125, 129)     # 2^-2 .. 2^2
WMAX = 6.0 * 4.0             # the largest |weight| of the exact cases
XMAX = 2                     # |staged activation| <= 2


def dequant64(codes, scales):
    """float64 [N][K] of codes [N][K] (0..15) and scale bytes [N][K/32]: exact for every byte 1..254."""
    v = mx.GRID.astype(np.float64)[codes & 7] * np.where(codes & 8, -1.0, 1.0)
    e = np.repeat(scales.astype(np.int64) - 127, mx.BLOCK, axis=1)
    return np.ldexp(v, e)


def exact_inputs(N, K, B, norm, seed):
    """Codes over the whole e2m1 grid with both signs (every one of the 16 codes occurs in every row of 32 or more
    columns), scale bytes in 125..129, norm_w 1 or 2 and integer x with |x * norm_w| <= 2: fp16(x norm_w) is the
    value itself, so the lo half is zero, and every term is a multiple of GRAIN = 2^-3 with |sum| <= K * 24 * 2 (at K
    4096: 196608 = 1.57 M grains < 2^24), so every partial sum is exact in fp32 in any order. Returns codes, scales,
    x, norm_w (None without a norm)."""
    r = np.random.default_rng(seed)
    codes = r.integers(0, 16, (N, K)).astype(np.uint8)
    # every code in both nibbles of a byte, rotated per row (at K 32 identical rows would leave the sums with one
    # mantissa pattern, and the fp32 norm factor could not be told from its neighbour)
    rot = np.arange(N)[:, None]
    codes[:, :16] = (np.arange(16)[None, :] + rot) % 16
    codes[:, 16:32] = (np.arange(16)[::-1][None, :] + 3 * rot) % 16
    scales = r.integers(SCALE_BYTES[0], SCALE_BYTES[1] + 1, (N, K // 32)).astype(np.uint8)
    norm_w = (2.0 ** r.integers(0, 2, K)).astype(np.float32) if norm else None
    lim = XMAX if norm_w is None else (XMAX // norm_w.astype(np.int64))[None, :]
    x = (r.integers(-XMAX, XMAX + 1, (B, K)).clip(-lim, lim)).astype(np.float32)
    return codes, scales, x, norm_w


def case(N, K, B, norm, seed):
    """A bgemm_ref case dict of exact_inputs, with the bound of the exact claim asserted on the inputs."""
    codes, scales, x, nw = exact_inputs(N, K, B, norm, seed)
    W = dequant64(codes, scales)
    h = R.staged(x, nw)
    assert np.abs(h).max() <= XMAX and np.array_equal(h, np.rint(h))
    hi, lo = R.P.split(h)
    assert not lo.any()  # the lo half is zero: the sums are those of the hi column alone
    Y, A = R.sums(W, x, nw)
    assert A.max() <= K * WMAX * XMAX and A.max() / GRAIN < 2 ** 24
    assert np.array_equal(Y / GRAIN, np.rint(Y / GRAIN)) and R.is_f32(Y)
    inv = R.inv_rms(x, R.EPS) if norm else None
    for a in (codes, scales, x, W, Y, A):
        a.setflags(write=False)
    return dict(W=W, scale=None, x=x, nw=nw, Y=Y, A=A, inv=inv, N=N, K=K, B=B, exact=True, codes=codes,
                data=mx.pack(codes), scales=scales)


def real_case(N, K, B, norm, seed, quant):
    """N(0, 1) activations, N(0, 1/K) weights quantised by `quant` (fp32 [N][K] -> data uint8 [N][K/2], scales uint8
    [N][K/32]: the device quantiser, itself held to mxfp4_ref bit for bit by test_gpu_mxfp4.py), norm weights 1 + 0.1 N.
    The reference sums are float64 over the dequantised weights."""
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, K)).astype(np.float32)
    wf = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    nw = (1 + 0.1 * r.standard_normal(K)).astype(np.float32) if norm else None
    data, scales = quant(wf)
    codes = mx.unpack(data)
    W = dequant64(codes, scales)
    Y, A = R.sums(W, x, nw)
    inv = R.inv_rms(x, R.EPS) if norm else None
    return dict(W=W, scale=None, x=x, nw=nw, Y=Y, A=A, inv=inv, N=N, K=K, B=B, exact=False, codes=codes, data=data,
                scales=scales)


# ---------------------------------------------------------------- the scale range
EXTREME = {1: ("min", 1.0), 253: ("max", 3.0), 254: ("max", 1.5)}  # byte: |code value| >= 1, <= 3, <= 1.5


def scale_range_case(N=256, K=256):
    """Scale bytes sweeping 1..254 across rows and blocks, every code elsewhere; at the extreme bytes the codes are
    restricted so that every weight is finite and a normal fp32: byte 1 (2^-126) only with |code value| >= 1, byte 253
    with <= 3, byte 254 with <= 1.5 (6 * 2^127 and 3 * 2^127 overflow; 0.5 * 2^-126 is subnormal)."""
    nb = K // 32
    scales = ((np.arange(N)[:, None] * nb + np.arange(nb)[None, :] * 37) % 254 + 1).astype(np.uint8)
    assert set(np.unique(scales)) == set(range(1, 255))
    codes = ((np.arange(N)[:, None] * 5 + np.arange(K)[None, :]) % 16).astype(np.uint8)
    # (code 8 is -0: a dot product that starts from +0 returns +0 for it, not the -0 of the table, so the one-hot
    # comparison of bit patterns leaves it out; its decode is covered by the exact cases, where it adds nothing)
    codes = np.where(codes == 8, 0, codes).astype(np.uint8)
    mag = mx.GRID[codes & 7]
    sb = np.repeat(scales, 32, axis=1)
    codes = np.where((sb == 1) & (mag < 1.0), (codes & 8) | 2, codes)            # -> +-1
    codes = np.where((sb == 253) & (mag > 3.0), (codes & 8) | 5, codes)          # -> +-3
    codes = np.where((sb == 254) & (mag > 1.5), (codes & 8) | 3, codes).astype(np.uint8)  # -> +-1.5
    return codes, scales
