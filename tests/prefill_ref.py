"""float64 numpy restatements of the prefill stages (simplellminference_amd/csrc/prefill.h), in the manner of
refmath.py: RMSNorm + hi/lo split, the GEMM with its three fused epilogues, block-causal attention. Plus the input
generators and the error bounds that tests/test_gpu_prefill_kernels.py holds the HIP kernels to, so the CPU suite
(test_prefill_ref_cpu.py) can check reference and generators against the C oracle before a GPU sees them.

Layouts (prefill.h): W [N][K] row-major; q/k/v rows [q heads; k heads; v heads], row = head * hd + d; one layer's
cache [hkv][T][hd]; gate/up rows [gate (inter); up (inter)].
"""
from __future__ import annotations

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)  # 2^-23
U32 = EPS32 / 2                          # unit roundoff of one fp32 operation
SPLIT_REL = 2.0 ** -22                   # hi + lo carries an fp32 value to 2^-22 relative (prefill.h pf_split) ...
SPLIT_ABS = 2.0 ** -24                   # ... and no finer than the smallest fp16 subnormal


# ---------------------------------------------------------------- 1. norm + split
def norm(x, w, eps):
    """rms_kernel.cpp:5-23 per row of x [M][D] (w None: x itself), float64."""
    x = np.asarray(x, np.float64)
    if w is None:
        return x
    return x / np.sqrt(np.mean(x * x, axis=1, keepdims=True) + eps) * np.asarray(w, np.float64)


def split(h32):
    """pf_split of fp32 values: hi = fp16(h), lo = fp16(h - hi) (h - hi is exact in fp32)."""
    h32 = np.asarray(h32, np.float32)
    hi = h32.astype(np.float16)
    lo = (h32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def joined(hi, lo):
    return np.asarray(hi, np.float64) + np.asarray(lo, np.float64)


# ---------------------------------------------------------------- 2. GEMM
def gemm_sums(W, hi, lo):
    """Y[m][r] = sum_k W[r][k] (hi[m][k] + lo[m][k]), float64 (W as stored: fp16 values or int8 integers)."""
    return joined(hi, lo) @ np.asarray(W, np.float64).T


def gemm_abs(W, hi, lo):
    """sum_k |W| (|hi| + |lo|): the magnitude every summation-order bound scales with."""
    return (np.abs(np.asarray(hi, np.float64)) + np.abs(np.asarray(lo, np.float64))) @ np.abs(np.asarray(W, np.float64)).T


def _scale(scale, n):
    return np.ones(n) if scale is None else np.asarray(scale, np.float64)


def rope_rows(a, pos, sin_t, cos_t, hd):
    """rope_kernel.cpp:22-41 on rows a [M][heads * hd] at positions pos [M] (rotate-half per head)."""
    M = a.shape[0]
    v = np.asarray(a, np.float64).reshape(M, -1, hd)
    h = hd // 2
    s = np.asarray(sin_t, np.float64)[pos][:, None, :]
    c = np.asarray(cos_t, np.float64)[pos][:, None, :]
    out = np.empty_like(v)
    out[..., :h] = v[..., :h] * c - v[..., h:] * s
    out[..., h:] = v[..., h:] * c + v[..., :h] * s
    return out.reshape(M, -1)


def rope_abs(a, pos, sin_t, cos_t, hd):
    """|a0||cos| + |a1||sin| per output of rope_rows: what its three fp32 roundings scale with."""
    M = a.shape[0]
    v = np.abs(np.asarray(a, np.float64)).reshape(M, -1, hd)
    h = hd // 2
    s = np.abs(np.asarray(sin_t, np.float64))[pos][:, None, :]
    c = np.abs(np.asarray(cos_t, np.float64))[pos][:, None, :]
    out = np.empty_like(v)
    out[..., :h] = v[..., :h] * c + v[..., h:] * s
    out[..., h:] = v[..., h:] * c + v[..., :h] * s
    return out.reshape(M, -1)


def epi_qkv(Y, scale, sin_t, cos_t, p0, nv, T, hq, hkv, hd):
    """PgEpiQKV (model.cpp:52-67): row scale, RoPE of the q and k rows at min(p0 + m, T - 1); q for every chunk
    row. Returns q [M][hq hd], k [M][hkv][hd], v [M][hkv][hd] and stored [M]: the rows m < nv with p0 + m < T,
    which alone reach the cache (at position p0 + m)."""
    M = Y.shape[0]
    a = np.asarray(Y, np.float64) * _scale(scale, Y.shape[1])
    pos = np.minimum(p0 + np.arange(M), T - 1)
    nq, nk = hq * hd, hkv * hd
    q = rope_rows(a[:, :nq], pos, sin_t, cos_t, hd)
    k = rope_rows(a[:, nq:nq + nk], pos, sin_t, cos_t, hd).reshape(M, hkv, hd)
    v = a[:, nq + nk:].reshape(M, hkv, hd)
    m = np.arange(M)
    stored = (m < nv) & (p0 + m < T)
    return q, k, v, stored


def act(g, u, silu):
    """swiglu_kernel.cpp:12-13: sigmoid(g) * u, or SiLU(g) * u."""
    sg = 1.0 / (1.0 + np.exp(-np.asarray(g, np.float64)))
    return (g * sg if silu else sg) * u


def epi_swiglu(Y, scale, inter, silu):
    a = np.asarray(Y, np.float64) * _scale(scale, Y.shape[1])
    return act(a[:, :inter], a[:, inter:], silu)


def epi_resid(Y, scale, resid):
    p = np.asarray(Y, np.float64) * _scale(scale, Y.shape[1])
    return p if resid is None else np.asarray(resid, np.float64) + p


# ---------------------------------------------------------------- 3. attention
def attn(q, K, V, p0, hq, hkv, hd, rows=None):
    """mha_kernel.cpp:36-77 per chunk row: row m of head h over cache rows 0 .. p0 + m of kv head h / (hq / hkv).
    q [M][hq hd], K / V [hkv][T][hd]. Rows at positions >= T are NaN (the kernels' result there means nothing)."""
    M = q.shape[0] if rows is None else rows
    T = K.shape[1]
    g = hq // hkv
    q = np.asarray(q, np.float64)
    K = np.asarray(K, np.float64)
    V = np.asarray(V, np.float64)
    out = np.full((M, hq * hd), np.nan)
    for m in range(M):
        pos = p0 + m
        if pos >= T:
            break
        for h in range(hq):
            s = K[h // g, :pos + 1] @ q[m, h * hd:(h + 1) * hd] / np.sqrt(hd)
            p = np.exp(s - s.max())
            out[m, h * hd:(h + 1) * hd] = (p / p.sum()) @ V[h // g, :pos + 1]
    return out


# ---------------------------------------------------------------- inputs on a dyadic grid
GRID_W = 64   # W = k / 64 (fp16) or W = k with power-of-two row scales (int8), k in [-8, 8]
GRID_H = 8    # hi and lo = k / 8, k in [-8, 8], independent draws


def grid_inputs(N, K, M, int8, seed):
    """Operands whose products and partial sums are exact in fp32 in any order: every term W (hi + lo) is a
    multiple of 1 / (GRID_W GRID_H) (int8: of 1 / GRID_H), and sum |W| (|hi| + |lo|) in those units stays below
    2^24 (grid_units checks it). hi and lo are independent, so losing or misplacing a lo image is an O(1) error,
    not a 2^-11 one. Returns W (fp16, or int8), row scales (None, or fp32 powers of two 2^-5 .. 2^-7), hi, lo."""
    r = np.random.default_rng(seed)
    k = r.integers(-8, 9, (N, K))
    if int8:
        W = k.astype(np.int8)
        scale = (2.0 ** -r.integers(5, 8, N)).astype(np.float32)
    else:
        W = (k / GRID_W).astype(np.float16)
        scale = None
    hi = (r.integers(-8, 9, (M, K)) / GRID_H).astype(np.float16)
    lo = (r.integers(-8, 9, (M, K)) / GRID_H).astype(np.float16)
    return W, scale, hi, lo


def grid_units(W, hi, lo):
    """max over outputs of sum |W| (|hi| + |lo|), in units of the grid step of one product (an integer)."""
    step_w = 1.0 if W.dtype == np.int8 else 1.0 / GRID_W
    return float(gemm_abs(W, hi, lo).max() / (step_w / GRID_H))


def grid_resid(M, N, seed):
    """An integer-grid residual: resid + sum stays exact in fp32."""
    return np.random.default_rng(seed).integers(-8, 9, (M, N)).astype(np.float32)


# ---------------------------------------------------------------- bounds (derivations: test_gpu_prefill_kernels.py)
def rope_tol(a, pos, sin_t, cos_t, hd, da=None):
    """|fp32 RoPE - exact RoPE| for inputs a known to +- da: fl(fl(a0 c) -+ fl(a1 s)) has three roundings,
    <= u A + u A (1 + u) < 1.5 eps32 A with A = |a0||c| + |a1||s|; an input error passes through with the same
    weights (|c|, |s| <= 1)."""
    t = 1.5 * EPS32 * rope_abs(a, pos, sin_t, cos_t, hd)
    if da is not None:
        t = t + rope_abs(da, pos, sin_t, cos_t, hd) * (1 + 2 * EPS32)
    return t


def act_tol(g, u, silu, dg=None, du=None):
    """|hi + lo - exact act| for exact fp32 g, u (or known to +- dg, du). fp32 chain of the kernel: expf (<= 2 ulp
    = 4 u relative on e, e / (1 + e) <= 1 of it on the result), 1 + e (u), the division (u), sg * up (u), SiLU's
    g * sg (u): <= 8 u = 4 eps32 relative; the hi/lo split adds 2^-22 relative, or one fp16 subnormal step where
    the result is that small. Input errors: |d act / d g| <= |u| / 4 (sigmoid) or 1.1 |u| (SiLU), |d act / d u| =
    |act(g, 1)|."""
    ref = np.abs(act(g, u, silu))
    t = (4 * EPS32 + SPLIT_REL) * ref + SPLIT_ABS
    if dg is not None:
        t = t + (1.1 if silu else 0.25) * np.abs(u) * dg + np.abs(act(g, np.ones_like(u), silu)) * du
    return t


def within_f16_rounding(got16, ref, tol):
    """got16 (fp16) is the round-to-nearest of some value within ref +- tol: rounding is monotone, so
    fp16(ref - tol) <= got <= fp16(ref + tol). With tol below an fp16 ulp that is the rounded reference or its
    neighbour on the side the fp32 error went."""
    got = np.asarray(got16, np.float64)
    lo = (np.asarray(ref, np.float64) - tol).astype(np.float16).astype(np.float64)
    hi = (np.asarray(ref, np.float64) + tol).astype(np.float16).astype(np.float64)
    return (lo <= got) & (got <= hi)
