"""Inputs for the MXFP4 prefill GEMM tests (simplellminference_amd/csrc/prefill.h pgemm_kernel, MXFP4 format): weights as
4-bit codes and e8m0 block scales (tests/mxfp4_ref.py layout) whose sums with k/8 activations are exact in fp32 in
any order, and the list of cases tests/test_gpu_mxfp4_prefill.py runs, so the CPU suite
(test_mxfp4_prefill_ref_cpu.py) can check every one of them against the condition before a GPU sees it.

Why the sums are exact: a row's block exponents lie in a window of `window` binades [e0, e0 + window). Every weight is
a multiple of 2^(e0 - 1) (the e2m1 grid step is 1/2) and at most 6 * 2^(e0 + window - 1) = 12 * 2^(window - 1) such
steps; hi and lo are multiples of 1/8, |hi| + |lo| <= 16 steps. So every product is an integer in units of
2^(e0 - 4), and a row's sum of magnitudes is at most K * 12 * 2^(window - 1) * 16 units: 6144 K at window 6 (6.3 M
at K = 1024), 3072 K at window 5 (6.3 M at K = 2048), below 2^24. Every partial sum in any order is then an integer
below 2^24 times one power of two: exact in fp32.
"""
from __future__ import annotations

import numpy as np

from tests import mxfp4_ref as mx
from tests import prefill_ref as R

CENTRE = -7                      # block exponents are drawn around 2^-7
MS = (32, 64, 128, 256)
DEPTHS = (64, 128, 192, 320, 704, 2048)  # 128-k stages: half, 1, 1.5, 2.5, 5.5, 16 stages
QKV = dict(hq=15, hkv=3, hd=64)     # N = 1344
QKV128 = dict(hq=6, hkv=2, hd=128)  # N = 1280
INTER = 576                         # N = 1152
N_RESID = 1168
RANGE_CENTRES = (-100, -40, -17, 0, 12, 40, 100)  # row r: RANGE_CENTRES[r % 7]; most lie outside fp16's range


def window_for(K):
    return 5 if K >= 2048 else 6


def grid_inputs(N, K, M, seed, window=None, centres=None):
    """codes uint8 [N][K] uniform over all 16, scale bytes uint8 [N][K/32] with exponents drawn per block from
    [c - window // 2, c - window // 2 + window) around the row's centre c (CENTRE, or centres[r]), hi and lo fp16
    [M][K], independent draws of k / 8, k in [-8, 8]."""
    window = window_for(K) if window is None else window
    r = np.random.default_rng(seed)
    codes = r.integers(0, 16, (N, K)).astype(np.uint8)
    c = np.full(N, CENTRE) if centres is None else np.asarray(centres)
    e = c[:, None] - window // 2 + r.integers(0, window, (N, K // mx.BLOCK))
    scales = (e + 127).astype(np.uint8)
    assert ((e + 127 >= 1) & (e + 127 <= 254)).all()
    hi = (r.integers(-8, 9, (M, K)) / R.GRID_H).astype(np.float16)
    lo = (r.integers(-8, 9, (M, K)) / R.GRID_H).astype(np.float16)
    return codes, scales, hi, lo


def range_centres(N):
    return np.array([RANGE_CENTRES[r % 7] for r in range(N)])


def weights64(codes, scales):
    """The weights as float64 (mxfp4_ref.dequantize is exact in fp32: byte 1 .. 254 scales of e2m1 values)."""
    return mx.dequantize(codes, scales).astype(np.float64)


def grid_units(codes, scales, hi, lo):
    """max over outputs of sum |W| (|hi| + |lo|) in units of the row's product grid step, 2^(e_min(row) - 4)."""
    W = weights64(codes, scales)
    emin = scales.astype(np.int64).min(axis=1) - 127
    return float((R.gemm_abs(W, hi, lo) / np.exp2(emin - 4.0)[None, :]).max())


def cell_cases(role, M):
    """(N, K, seed) of every grid GEMM the exact-sum test runs for one picker cell (role, chunk size)."""
    out = []
    for K in DEPTHS:
        seed = 1000 * K + 10 * M + role
        if role == 2:
            out.append((N_RESID, K, seed))
        elif role == 1:
            out.append((2 * INTER, K, seed))
        else:
            out.append((1344, K, seed + 1344))
            if K == 192:
                out.append((1280, K, seed + 1280))
    return out


def all_grid_cases():
    """Every (N, K, M, seed, centres) the GPU tests draw grid inputs with."""
    cases = [(N, K, M, seed, None) for role in (0, 1, 2) for M in MS for N, K, seed in cell_cases(role, M)]
    cases.append((N_RESID, 704, 64, 77, range_centres(N_RESID)))                 # scale range
    cases += [(N_RESID, K, 32, 500 + K, None) for K in (64, 192, 704)]           # stays inside its operands
    cases += [(1344, 128, 64, 7 + case, None) for case in range(4)]              # cache-store bounds
    return cases
