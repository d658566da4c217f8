"""float64 numpy restatement of ONE batched decode projection launch (simplellminference_amd/csrc/bgemm.h
bgemm_kernel), in the manner of prefill_ref.py, plus the input generators and error bounds that
tests/test_gpu_batch_kernels.py holds the kernel to. test_bgemm_ref_cpu.py checks all of it against the C oracle
before a GPU sees it.

The launch, for B <= 8 sequences x [B][K] fp32 and W [N][K] (fp16 values or int8 integers):
  h[b]    = x[b]                                   (store: wo / down), or
            fl32(x[b] * norm_w)                    (q/k/v, gate/up, logits: the fused RMSNorm stages x * w ...)
  inv[b]  = 1 / sqrt(mean(x[b]^2) + eps)           (... and its per-sequence factor multiplies the finished sum:
                                                    rms_kernel.cpp:12-19; a scalar commutes with the k-sum)
  hi, lo  = fp16(h), fp16(h - hi)                  (the fp32 operand carried on two MFMA columns)
  Y[b][r] = sum_k W[r][k] (hi + lo)[b][k]
  a[b][r] = Y[b][r] * inv[b] * row_scale[r]        (in that order)
then one of four epilogues (layouts as bgemm.h: q/k/v rows [q heads; k heads; v heads], one layer's cache
[B][hkv][T][hd], gate/up rows [gate (inter); up (inter)]).

Reused as they are: prefill_ref rope_rows / rope_tol / act / act_tol / within_f16_rounding / split (the same
arithmetic), kv8_ref encode / MIDS for the FP8 cache; test_bgemm_ref_cpu.py also holds it to refmath's operators.
"""
from __future__ import annotations

import numpy as np

from tests import kv8_ref as F8
from tests import prefill_ref as P

EPS32, U32, SPLIT_REL = P.EPS32, P.U32, P.SPLIT_REL
NORM_RTOL = 2e-6  # test_rmsnorm's bar on the fp32 RMS factor


# ---------------------------------------------------------------- the launch
def inv_rms(x, eps):
    """rms_kernel.cpp:12-19 per sequence: mean square, + eps, sqrt, reciprocal. float64 [B]."""
    x = np.asarray(x, np.float64)
    return 1.0 / np.sqrt(np.mean(x * x, axis=1) + eps)


def staged(x, norm_w):
    """The fp32 rows the kernel stages: x, or the fp32 product x * norm_w (one rounding)."""
    x = np.asarray(x, np.float32)
    return x if norm_w is None else x * np.asarray(norm_w, np.float32)[None, :]


def sums(W, x, norm_w):
    """Y [B][N] float64 over the staged operand as the MFMA sees it (hi + lo), and A = |W| @ |h|."""
    hi, lo = P.split(staged(x, norm_w))
    return P.gemm_sums(W, hi, lo), P.gemm_abs(W, hi, lo)


def scaled(Y, inv, scale):
    """a = Y * inv[b] * row_scale[r] (inv None: no norm; scale None: no row scale)."""
    a = np.asarray(Y, np.float64)
    if inv is not None:
        a = a * np.asarray(inv, np.float64)[:, None]
    if scale is not None:
        a = a * np.asarray(scale, np.float64)[None, :]
    return a


def epi_qkv(a, pos, sin_t, cos_t, hq, hkv, hd):
    """BgEpiQKV (model.cpp:54-67): RoPE of sequence b's q and k rows at pos[b]. q [B][hq hd], k, v [B][hkv][hd]."""
    B = a.shape[0]
    nq, nk = hq * hd, hkv * hd
    pos = np.asarray(pos)
    q = P.rope_rows(a[:, :nq], pos, sin_t, cos_t, hd)
    k = P.rope_rows(a[:, nq:nq + nk], pos, sin_t, cos_t, hd).reshape(B, hkv, hd)
    return q, k, a[:, nq + nk:].reshape(B, hkv, hd)


def epi_swiglu(a, inter, silu):
    return P.act(a[:, :inter], a[:, inter:], silu)


def epi_store(a, resid, scale):
    p = a * float(scale)
    return p if resid is None else np.asarray(resid, np.float64) + p


def ordered(v32):
    """common.h argmax_key's orderable image of fp32 values (uint32): -0 counts as +0, larger float, larger image."""
    u = np.asarray(v32, np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def argmax_key(v32, idx):
    return (ordered(v32) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(idx, np.uint64))


def key_parts(key):
    key = np.asarray(key, np.uint64)
    return key >> np.uint64(32), np.uint64(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF))


def best_key(row32, vocab_off):
    """The key of a logits row: its maximum and, among equals (+-0 included), the lowest index."""
    o = ordered(row32)
    i = int(np.argmax(o))  # first occurrence of the maximum
    return int(argmax_key(row32[i], i + vocab_off))


# ---------------------------------------------------------------- bounds
def sum_tol(A, K):
    """|fp32 MFMA sum - float64 sum of the identical rounded operands|: 4 eps32 sqrt(K) A (test_matmul_f32's bound,
    bar (c) of the prefill tests) plus the hi/lo carry of the fp32 operand, 2^-22 A."""
    return (4 * EPS32 * np.sqrt(K) + SPLIT_REL) * A


def scaled_tol(Y, dY, inv, scale):
    """da for a = Y inv scale with Y known to +- dY and the fp32 inv to NORM_RTOL; each of the two multiplies
    rounds once."""
    a = np.abs(scaled(Y, inv, scale))
    da = np.abs(scaled(dY, inv, scale))
    if inv is not None:
        da = da + (NORM_RTOL + U32) * a
    if scale is not None:
        da = da + U32 * a
    return da


def swiglu_tol(g, u, silu, dg=None, du=None):
    """prefill_ref.act_tol without its hi/lo split terms: the batched kernel stores the fp32 activation itself."""
    t = P.act_tol(g, u, silu, dg, du) - SPLIT_REL * np.abs(P.act(g, u, silu)) - P.SPLIT_ABS
    return t + 1e-45  # (an exact zero activation: 0 <= 0)


def f8_accept(ref, tol):
    """FP8 codes a correct kernel may store for a value known as ref +- tol: encode(ref), or where the interval
    straddles a code boundary (kv8_ref.MIDS) the neighbouring code. Returns (codes of ref, lo codes, hi codes): a
    stored code is right when it lies between encode(ref - tol) and encode(ref + tol) in value order."""
    ref = np.asarray(ref, np.float64)
    return F8.encode(ref), F8.encode(ref - tol), F8.encode(ref + tol)


def f8_check(got, ref, tol):
    """(ok mask, used-the-neighbour mask). Value order of the codes: decode is monotone in the value."""
    ref = np.asarray(ref, np.float64)
    want, lo, hi = f8_accept(ref, tol)
    got = np.asarray(got, np.uint8)
    gv, lv, hv = F8.TABLE64[got], F8.TABLE64[lo], F8.TABLE64[hi]
    exact = got == want
    # a zero code carries the value's sign: the other zero only where the interval holds values of that sign
    sign_ok = (gv != 0) | np.where(got & 0x80, ref - tol <= 0, ref + tol >= 0)
    ok = exact | ((lv <= gv) & (gv <= hv) & sign_ok)
    return ok, ok & ~exact


# ---------------------------------------------------------------- exact inputs
def row_scale_pow2(n):
    """2^((r % 5) - 2): 1/4 .. 4 (test_gpu_batch_i8.py)."""
    return (2.0 ** ((np.arange(n) % 5) - 2)).astype(np.float32)


RANGES = ((15, 2), (7, 2), (3, 2), (3, 1), (1, 1))  # (|W| <=, |a| <=), narrowed at depth until the sums are exact


def exact_inputs(N, K, B, int8, family, norm, seed):
    """Operands whose products and partial sums are exact in fp32 in ANY order. W: integers (fp16 values, or int8
    with the power-of-two row scales). x, family "int": integers in [-4 amax, 4 amax]; family "lo": a + c 2^-12 with
    integer |a| <= amax and c in {-1, 0, 1}, so fp16(x) = a (or c 2^-12 where a = 0) and the lo column carries
    c 2^-12: dropping it changes most outputs. norm_w: 1 or 2, so x * norm_w is exact. The ranges are the widest of
    RANGES for which sum |W| |x norm_w|, in units of the grid step of one term, stays below 2^24 for every output:
    then every partial sum is an integer below 2^24 in those units. Returns W, row scales (None for fp16), x,
    norm_w (None without a norm)."""
    for wmax, amax in RANGES:
        r = np.random.default_rng(seed)
        k = r.integers(-wmax, wmax + 1, (N, K))
        W = k.astype(np.int8) if int8 else k.astype(np.float16)
        if family == "int":
            x = r.integers(-4 * amax, 4 * amax + 1, (B, K)).astype(np.float32)
        else:
            x = (r.integers(-amax, amax + 1, (B, K)) + r.integers(-1, 2, (B, K)) * 2.0 ** -12).astype(np.float32)
        norm_w = (2.0 ** r.integers(0, 2, K)).astype(np.float32) if norm else None
        if exact_units(W, x, norm_w, family) < 2 ** 24:
            return W, (row_scale_pow2(N) if int8 else None), x, norm_w
    raise AssertionError(f"no range keeps the sums of a {N} x {K} case exact")


def exact_units(W, x, norm_w, family):
    """max over outputs of sum |W| |x norm_w| in grid units, after checking that the staged operand is exact:
    x * norm_w has no rounding and hi + lo carries it whole."""
    unit = 1.0 if family == "int" else 2.0 ** -12
    h = staged(x, norm_w)
    h64 = np.asarray(x, np.float64) * (1.0 if norm_w is None else np.asarray(norm_w, np.float64)[None, :])
    assert np.array_equal(h.astype(np.float64), h64)
    hi, lo = P.split(h)
    assert np.array_equal(P.joined(hi, lo), h64)
    units = P.gemm_abs(W, hi, lo).max() / unit
    assert units == np.round(units)
    return float(units)


def lo_matters(W, x, norm_w):
    """Share of the outputs that change when the lo column is dropped."""
    hi, lo = P.split(staged(x, norm_w))
    return float(np.mean(P.gemm_sums(W, hi, np.zeros_like(lo)) != P.gemm_sums(W, hi, lo)))


def exact_resid(B, ld, seed):
    return np.random.default_rng(seed).integers(-8, 9, (B, ld)).astype(np.float32)


def is_f32(a):
    """Every value of a float64 array is an fp32 number: an fp32 operation with this exact result does not round."""
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


def inv_candidates(inv64, ulps=4):
    """The fp32 numbers within `ulps` ulp of the float64 factor, ascending."""
    c = np.float32(inv64)
    out = [c]
    lo = hi = c
    for _ in range(ulps):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return sorted(set(out))


def apply_inv(Y_row, inv32, scale):
    """fl32(fl32(sum * inv) * row scale) for exact sums Y_row (fp32 numbers): what the kernel stores."""
    v = np.asarray(Y_row, np.float32) * np.float32(inv32)
    return v if scale is None else v * np.asarray(scale, np.float32)


def recover_inv(got_rows, Y_rows, inv64, scale):
    """The one fp32 factor within 4 ulp of inv64 that reproduces EVERY given output of a sequence bit for bit from
    its exact sums, or None. (Zero sums are reproduced by any factor: the caller gives rows with non-zero sums.)"""
    hits = [c for c in inv_candidates(inv64) if np.array_equal(apply_inv(Y_rows, c, scale), got_rows)]
    return hits[0] if len(hits) == 1 else None


# ---------------------------------------------------------------- the cells the GPU file runs
QKV64 = dict(hq=4, hkv=2, hd=64)     # N 512, 32 tiles
QKV128 = dict(hq=2, hkv=1, hd=128)   # N 512
QKV_WIDE = dict(hq=7, hkv=1, hd=64)  # N 576, 36 tiles: 17 + 17 + 2
INTER, INTER_WIDE = 40, 280          # 5 tiles; 35 tiles
NROWS, LD, NROWS_WIDE, LD_WIDE = 70, 96, 550, 552  # 5 tiles, the last clamped; 35 tiles, the last clamped
VOCAB_OFF = 1000
T = 40
EPS = 1e-5
# depth K -> k-blocks per wave: 32: one block, 15 idle waves; 544: 17 blocks, 1 or 2 per wave, K % 64 != 0; 2560: 5
# (width 4: a full step, then a clamped one; width 2: 2 + 2 + 1, staging ends on a half-filled pair); 4096: 8 (every
# staging register, the LDS image near its limit)
DEPTHS = (32, 544, 2560, 4096)
PLANS = ((1, 1), (2, 1), (3, 1))  # width 2; width 4 with a short last workgroup (5 tiles, or 32 over 3)
WRAP = (17, 1)                    # tiles j and j + 16 reduced by one wave, the P double buffer wraps
# store only, (K, tpw, splits): 1792: 3 or 4 blocks per wave at width 2; the width-7 path: 3584 (7 per wave), 3072 (6,
# one clamped duplicate), 7168 and 6144 over 2 splits (7 and 6 per wave plus the split merge); 1024 over 2 splits: one
# block per wave and split at widths 2 and 4; 2816 over 4 splits: 22 blocks a split, 1 or 2 per wave at width 2
STORE_EXTRA = ((1792, 1, 1), (3584, 2, 1), (3584, 3, 1), (3072, 2, 1), (7168, 2, 2), (6144, 2, 2), (1024, 1, 2),
               (1024, 2, 2), (2816, 1, 4))


def cells(role):
    """(shape, K, tpw, splits) of every forced plan the GPU file runs for a role ("qkv", "gate_up", "store",
    "logits"); shape is the geometry dict (qkv), inter, or (nrows, ld). The automatic plan runs besides."""
    small = {"qkv": QKV64, "gate_up": INTER, "store": (NROWS, LD), "logits": (NROWS, LD)}[role]
    wide = {"qkv": QKV_WIDE, "gate_up": INTER_WIDE, "store": (NROWS_WIDE, LD_WIDE), "logits": (NROWS_WIDE, LD_WIDE)}[role]
    out = [(small, K, tpw, s) for K in DEPTHS for tpw, s in PLANS]
    out.append((wide, 64) + WRAP)
    if role == "qkv":
        out += [(QKV128, K, tpw, s) for K in (544, 4096) for tpw, s in PLANS[:2]]
    if role == "logits":
        out.append((wide, 4096) + WRAP)  # the 8B LM head's class: 16 or more tiles with all 8 staged blocks per wave
    if role == "store":
        out += [(small, K, tpw, s) for K, tpw, s in STORE_EXTRA]
    return out


def rows_of(role, shape):
    if role == "qkv":
        return (shape["hq"] + 2 * shape["hkv"]) * shape["hd"]
    return 2 * shape if role == "gate_up" else shape[0]


def plan_class(plan, K, norm):
    """What a plan exercises: (step width, tiles per workgroup 1 / 2..15 / 16+, one split or more, norm, k-blocks per
    wave)."""
    tpw, s = plan["tpw"], plan["splits"]
    per_split = (K // 32 + s - 1) // s
    per_wave = (per_split + 15) // 16
    return (plan["step_width"], "1" if tpw == 1 else ("2..15" if tpw < 16 else "16+"), "1" if s == 1 else ">1",
            bool(norm), per_wave)


# ---------------------------------------------------------------- realistic inputs
def real_inputs(N, K, B, int8, norm, seed):
    """x standard normal, W ~ N(0, 1/K) as fp16 or per-row symmetric int8 (scale = amax / 127), norm_w = 1 + 0.1 N."""
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, K)).astype(np.float32)
    wf = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    norm_w = (1 + 0.1 * r.standard_normal(K)).astype(np.float32) if norm else None
    if not int8:
        return wf.astype(np.float16), None, x, norm_w
    s = (np.abs(wf).max(axis=1) / 127.0).astype(np.float32)
    return np.clip(np.rint(wf / s[:, None]), -127, 127).astype(np.int8), s, x, norm_w
