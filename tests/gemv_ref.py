"""float64 numpy restatement of ONE batch-1 decode GEMV launch (simplellminference_amd/csrc/gemv.h), in the manner of
bgemm_ref.py, plus the input generators, the error bounds and the list of cells that tests/test_gpu_decode_gemv.py
holds the kernels to through sli_decode_gemv (include/sli.h "decode stages, for tests and labs").
test_gemv_ref_cpu.py checks the arithmetic against the C oracle and test_decode_stage_cpu.py the cell list against the
schedules a production model runs, before a GPU sees either.

The launch, for x [K] fp32 and W [N][K] (fp32 / fp16 values, int8 integers with row scales, MXFP4 with block scales):
  h       = the staged input, fp32:
              x                                          (wo with a plain input, down)
              fl(fl(x * inv) * norm_w)                   (q/k/v, gate/up, logits: the norm is applied BEFORE the
              inv = fl(1 / sqrtf(fl(ss / K) + eps))       products, unlike bgemm's, which scales the finished sum)
              x1 = ((x + p_0) + p_1) + ... in fp32       (gate/up after a K-split wo: XStageSum, then the norm of x1)
              o / L, o = sum_s e^(m_s - M) o_s, L = sum_s e^(m_s - M) l_s over the ns = min(pos / ppwg + 1, max_splits)
              live splits in split order, M = max m_s    (wo: XStageMerge)
  sum[r]  = sum_k W[r][k] h[k]                           (fp32 fma chains per lane, a wave reduction, then the
                                                          column parts added in part order)
  a[r]    = fl(sum[r] * row_scale[r])
then one of the epilogues (EpiQKV, EpiSwiGLU, EpiStore / EpiStoreSum / EpiKPart, EpiLogits). The K-split residual is
x1 = ((x + p_0) + ...) + p_{NP-1} in that order, in XStageSum and EpiStoreSum alike: numpy fp32 adds reproduce it to
the bit, so x1 is an operand here, not a result with a bound.

Reused as they are: bgemm_ref (inv_rms, epi_*, argmax_key / best_key, f8_check, row_scale_pow2),
prefill_ref (rope_tol, act_tol, within_f16_rounding), mxfp4_ref, kv8_ref.
"""
from __future__ import annotations

import numpy as np

from tests import bgemm_ref as B
from tests import mxfp4_ref as MX
from tests import prefill_ref as P

EPS32, U32, NORM_RTOL = P.EPS32, P.U32, B.NORM_RTOL
WTS = ("f32", "f16", "i8", "mxfp4")
EPV = {"f32": 4, "f16": 8, "i8": 16, "mxfp4": 32}  # weight elements per 16-byte vector
WAVES = 16
QKV, GATE_UP, WO, DOWN, LOGITS = 0, 1, 2, 3, 4


# ---------------------------------------------------------------- the staged input
def x1_sum(x, parts):
    """XStageSum / EpiStoreSum: ((x + p_0) + p_1) + ... in fp32, that order. Bit-exact (IEEE adds)."""
    v = np.asarray(x, np.float32).copy()
    for p in (() if parts is None else parts):
        v = v + np.asarray(p, np.float32)
    return v


def staged_norm(x, norm_w, eps):
    """float64 of the normalised input, x * inv * w, and inv (float64)."""
    inv = float(B.inv_rms(np.asarray(x)[None, :], eps)[0])
    return np.asarray(x, np.float64) * inv * np.asarray(norm_w, np.float64), inv


def staged_norm_tol(h):
    """|fl(fl(x inv32) w) - x inv w|: the fp32 factor within NORM_RTOL of the float64 one, and two roundings."""
    return (NORM_RTOL + 2 * U32) * (1 + EPS32) * np.abs(h)


def live_splits(pos, ppwg, max_splits):
    return min(pos // ppwg + 1, max_splits)


def merge(part, ns, hd):
    """XStageMerge on part [heads][max_splits][hd + 4] (o[hd], m, l, pad): float64 h [heads * hd] over splits < ns, and
    its bound. fp32 chain of the kernel per element: m_s - M (one rounding: relative u |m_s - M| on the weight), expf
    (<= 2 ulp = 4 u), one fma per split into o and into L (<= ns u of sum w |o_s|, resp. of L: every term of L is
    positive), the division (u): |h32 - h| <= (5 + ns + max|m_s - M|) u (sum_s w_s |o_s| / L + |h|) + u |h|."""
    p = np.asarray(part, np.float64)[:, :ns]
    o, m, l = p[:, :, :hd], p[:, :, hd], p[:, :, hd + 1]
    M = m.max(axis=1, keepdims=True)
    w = np.exp(m - M)
    L = (w * l).sum(axis=1)
    h = (w[:, :, None] * o).sum(axis=1) / L[:, None]
    A = (w[:, :, None] * np.abs(o)).sum(axis=1) / L[:, None]
    c = (5 + ns + np.abs(m - M).max(axis=1))[:, None] * U32
    return h.reshape(-1), (c * (A + np.abs(h)) + U32 * np.abs(h)).reshape(-1)


# ---------------------------------------------------------------- sums and their bound
def w64(W, wt):
    """The weight values in float64: W as stored (fp32 / fp16 / int8 integers), or (packed data, scale bytes) for
    mxfp4."""
    if wt == "mxfp4":
        return MX.dequantize(MX.unpack(W[0]), W[1]).astype(np.float64)
    return np.asarray(W, np.float64)


def sums(Wv, h):
    """Y [N] float64 and A = |W| @ |h|."""
    h = np.asarray(h, np.float64)
    return Wv @ h, np.abs(Wv) @ np.abs(h)


def sum_tol(A, K):
    """|fp32 fma sum - float64 sum of the identical operands|: bgemm_ref.sum_tol without its hi/lo term (the GEMV
    stages fp32 itself): 4 eps32 sqrt(K) A."""
    return 4 * EPS32 * np.sqrt(K) * A


def kpart_view(Wv, ks):
    """EpiKPart's view of the [D][QD] wo matrix: [ks][D][QD / ks], block k = columns [k QD / ks, (k + 1) QD / ks)."""
    D, QD = Wv.shape
    return Wv.reshape(D, ks, QD // ks).transpose(1, 0, 2)


def scaled(Y, dY, scale):
    """a = fl(Y * row scale) and its bound."""
    if scale is None:
        return Y, dY
    s = np.asarray(scale, np.float64)
    return Y * s, dY * np.abs(s) + U32 * np.abs(Y * s)


def swiglu_tol(g, u, silu, dg, du):
    """prefill_ref.act_tol without its hi/lo split terms (the GEMV stores the fp32 activation itself), written out term
    by term: bgemm_ref.swiglu_tol subtracts the split terms from act_tol, which cancels the 4 eps32 |act| term away
    where the activation is far below 2^-24 (sigmoid of a sum near -60: the exact family's integer sums reach it).
    fp32 chain: expf (<= 2 ulp), 1 + e, the division, sg * up, SiLU's g * sg: <= 8 u = 4 eps32 relative; input errors
    through |d act / d g| <= |u| / 4 (sigmoid) or 1.1 |u| (SiLU) and |d act / d u| = |act(g, 1)|. Underflow, which
    act_tol leaves out: for g < -87.3 the sigmoid 1 / (1 + e^-g) lies below the smallest normal fp32 number 2^-126
    (and e^-g overflows to inf past 88.7, the quotient becoming 0), so it is known to 2^-126 absolute, not to a
    relative error; that passes through the factors g (SiLU) and u."""
    t = 4 * EPS32 * np.abs(P.act(g, u, silu)) + 2.0 ** -126 * (np.maximum(1.0, np.abs(g)) if silu else 1.0) * np.abs(u)
    return t + (1.1 if silu else 0.25) * np.abs(u) * dg + np.abs(P.act(g, np.ones_like(u), silu)) * du + 1e-45


# ---------------------------------------------------------------- exact inputs
def exact_x_norm(K, seed):
    """A signed shuffle of 11 K / 16 entries of magnitude 1 and 5 K / 16 of magnitude 7: sum x^2 = 16 K with every fp32
    partial sum an integer below 2^24 in ANY order, so fl(ss / K) = 16 and, with eps = 0, inv = 0.25 exactly."""
    assert K % 16 == 0 and 16 * K < 2 ** 24
    r = np.random.default_rng(seed)
    mag = np.concatenate([np.ones(11 * K // 16), np.full(5 * K // 16, 7.0)])
    x = (r.permutation(mag) * r.choice([-1.0, 1.0], K)).astype(np.float32)
    assert float(np.sum(x.astype(np.float64) ** 2)) == 16.0 * K
    ss = np.float32(0)
    for c in np.array_split(x * x, 64):  # one of the orders: per-chunk partials, then their sum
        ss = ss + np.float32(c.sum(dtype=np.float32))
    assert np.float32(1) / np.sqrt(ss / np.float32(K) + np.float32(0)) == np.float32(0.25)
    return x


def exact_norm_w(K, seed):
    return (2.0 ** np.random.default_rng(seed + 1).integers(0, 2, K)).astype(np.float32)


def exact_weights(N, K, wt, seed):
    """Integer weights: fp32 / fp16 values in [-4, 4]; int8 in [-4, 4] with bgemm_ref's power-of-two row scales; MXFP4
    grid values with block scales 2^-1 .. 2^1 (so every value is a multiple of 2^-2). Returns (W as the device takes
    it: array, or (data, scales) for mxfp4), row scales or None, the float64 values, the grid step of one value."""
    r = np.random.default_rng(seed)
    if wt == "mxfp4":
        codes = r.integers(0, 16, (N, K)).astype(np.uint8)
        sc = r.integers(126, 129, (N, K // 32)).astype(np.uint8)
        return (MX.pack(codes), sc), None, MX.dequantize(codes, sc).astype(np.float64), 0.25
    k = r.integers(-4, 5, (N, K))
    W = k.astype({"f32": np.float32, "f16": np.float16, "i8": np.int8}[wt])
    return W, (B.row_scale_pow2(N) if wt == "i8" else None), k.astype(np.float64), 1.0


def exact_units(Wv, h, unit):
    """max over outputs of sum |W| |h| in grid units (the products' common step); every term must be a multiple of it.
    Below 2^24, every fp32 partial sum of the products is exact in any order."""
    terms = np.abs(Wv) * np.abs(np.asarray(h, np.float64))[None, :] / unit
    assert np.array_equal(terms, np.round(terms)), "a product is off the grid"
    return float(terms.sum(axis=1).max())


def exact_parts(np_, n, seed):
    return np.random.default_rng(seed + 2).integers(-3, 4, (np_, n)).astype(np.float32)


BIG = 2.0 ** 25  # fp32 spacing 4 there: adding 1 or 7 to it rounds


def plant_order(x, parts, x1):
    """Every third element of (x, parts) replaced so that ((x + p_0) + p_1) + ... is still x1 exactly but any other
    order of the adds is not: x = -2^25, p_0 = 2^25, p_1 = x1 (np 4: p_2 = 1, p_3 = -1). In order, x + p_0 = 0 and the
    rest is exact; with p_0 added later, x1 (odd) is added to -2^25 and rounds to a multiple of 4."""
    i = np.arange(0, x.size, 3)
    x, parts = x.copy(), parts.copy()
    x[i], parts[0, i], parts[1, i] = -BIG, BIG, x1[i]
    if len(parts) == 4:
        parts[2, i], parts[3, i] = 1.0, -1.0
    assert np.array_equal(x1_sum(x, parts), x1) and (x1_sum(x, parts[::-1])[i] != x1[i]).all()
    return x, parts


def plant_order_resid(resid, parts):
    """The same for a residual that need not come out at a given value: resid = 2^25, p_last = -2^25, the parts
    between +-1: in order the ones are absorbed and the sum is 0; last to first it is their sum (odd or +-1)."""
    i = np.arange(0, resid.size, 3)
    resid, parts = resid.copy(), parts.copy()
    resid[i], parts[-1, i] = BIG, -BIG
    parts[:-1, i] = np.where(parts[:-1, i] >= 0, 1.0, -1.0)
    assert (x1_sum(resid, parts)[i] == 0).all() and (x1_sum(resid, parts[::-1])[i] != 0).all()
    return resid, parts


def exact_merge_parts(heads, max_splits, hd, ns, seed):
    """part [heads][max_splits][hd + 4] for the exact family: every live m_s equal (the weights are expf(0) = 1), l_s =
    1, 1, 2, 4, ... (power-of-two prefix sums), o_s integers in [-2, 2]: the merged input sum_s o_s / 2^(ns - 1) (ns
    1: / 1) is exact for every ns. Dead splits (s >= ns) and the pad words are NaN: consumed, they show."""
    r = np.random.default_rng(seed + 3)
    part = np.full((heads, max_splits, hd + 4), np.nan, np.float32)
    part[:, :ns, :hd] = r.integers(-2, 3, (heads, ns, hd))
    part[:, :ns, hd] = 1.5
    part[:, :ns, hd + 1] = np.array([1.0] + [2.0 ** max(s - 1, 0) for s in range(1, ns)], np.float32)[None, :]
    return part


def real_merge_parts(heads, max_splits, hd, ns, seed):
    """Realistic partials: o_s normal, distinct m_s, l_s in [1, ppwg]; dead splits and pads NaN. Every other head's
    split 0 lies 120 below the rest (a context whose first positions score far lower): its weight underflows, as it
    should, while a merge that took M from split 0 instead of the maximum would overflow expf (e^88.7)."""
    r = np.random.default_rng(seed + 3)
    part = np.full((heads, max_splits, hd + 4), np.nan, np.float32)
    part[:, :ns, :hd] = r.standard_normal((heads, ns, hd)) * 8
    part[:, :ns, hd] = r.standard_normal((heads, ns)) * 3
    part[::2, 0, hd] -= 120.0
    part[:, :ns, hd + 1] = r.uniform(1, 64, (heads, ns))
    return part


def real_weights(N, K, wt, seed):
    """W ~ N(0, 1 / K): fp32, fp16-rounded, per-row symmetric int8, or the MXFP4 rule of mxfp4_ref."""
    r = np.random.default_rng(seed)
    wf = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    if wt == "f32":
        return wf, None, wf.astype(np.float64)
    if wt == "f16":
        W = wf.astype(np.float16)
        return W, None, W.astype(np.float64)
    if wt == "i8":
        s = (np.abs(wf).max(axis=1) / 127.0).astype(np.float32)
        W = np.clip(np.rint(wf / s[:, None]), -127, 127).astype(np.int8)
        return W, s, W.astype(np.float64)
    codes, sc = MX.quantize(wf)
    return (MX.pack(codes), sc), None, MX.dequantize(codes, sc).astype(np.float64)


# ---------------------------------------------------------------- the schedule of a plan (gemv.h gemv_block)
def wave_items(plan):
    """Items ((unit, column part) pairs) of every streaming wave, per workgroup: gemv_block's partition."""
    G, N, cs, cw = plan["grid"], plan["units"], plan["csplit"], plan["cw"]
    out = []
    for b in range(G):
        ub, ue = (b * WAVES * N) // (G * WAVES), ((b + 1) * WAVES * N) // (G * WAVES)
        ni = (ue - ub) * cs
        out.append([((w + 1) * ni) // cw - (w * ni) // cw for w in range(cw)])
    return out


def schedule_class(role, plan):
    """What a launch exercises: (role, column parts, vectors per lane, more than one chunk per row, masked tail, most
    items of a wave 1 / 2 / 3+, waves of unequal item counts, waves with no item, fewer than 16 streaming waves, NS)."""
    cnt = [c for wg in wave_items(plan) for c in wg]
    return (role, plan["csplit"], plan["u"], plan["chunks_per_row"] > 1, bool(plan["masked_tail"]), min(max(cnt), 3),
            len({c for c in cnt if c > 0}) > 1, min(cnt) == 0, plan["cw"] < WAVES, plan["ns"])


# ---------------------------------------------------------------- production launches (test_decode_stage_cpu.py)
MODELS = {  # D, hq, hkv, hd, I, V
    "llama2-7b": (4096, 32, 32, 128, 11008, 32000),
    "llama3-8b": (4096, 32, 8, 128, 14336, 128256),
}
PRODUCTION = (("llama2-7b", 1), ("llama2-7b", 4), ("llama2-7b", 8), ("llama3-8b", 1))


def production_launches(model, tp):
    """(role, cols, shape) of every GEMV launch of a batch-1 step of the model's rank at tensor-parallel degree tp, in
    every variant the engine takes (engine.hip StepRecorder): wo plain (the attention merged), merged, and at TP 1
    K-split by 2 with its gate/up and down consumers."""
    D, hq, hkv, hd, I, V = MODELS[model]
    hq, hkv, I, V = hq // tp, hkv // tp, I // tp, V // tp
    qd = hq * hd
    out = [(QKV, D, dict(hq=hq, hkv=hkv, hd=hd, T=2048, kv_dtype=1)),
           (GATE_UP, D, dict(inter=I)),
           (WO, qd, dict(nrows=D)),
           (WO, qd, dict(nrows=D, merged=True, hq=hq, hd=hd, max_splits=8, ppwg=256)),
           (DOWN, I, dict(nrows=D)),
           (LOGITS, D, dict(nrows=V, key_ld=4096))]
    if tp == 1:
        out += [(WO, qd, dict(nrows=D, hq=hq, hd=hd, max_splits=8, ppwg=256, ks=2)),
                (GATE_UP, D, dict(inter=I, np=2)),
                (DOWN, I, dict(nrows=D, np=2))]
    return out


# ---------------------------------------------------------------- the cells the GPU file runs
# (role, cols, cus, shape): shape is what ops.decode_gemv_plan takes. Found with sli_decode_gemv_plan on the CPU: each
# keeps the production column count and scales the rows and the chip down together (cus / 256), so its plan has the
# schedule class of a production launch (test_decode_stage_cpu.py checks the cover, per weight type), or takes one
# of the branches listed beside it. Every cell runs for every weight type whose vector width divides its columns.
T = 40          # cache rows of the q/k/v cells
PPWG = 4        # positions per attention split of the merged-input cells (the partial buffer is the caller's)
VOCAB_OFF = 1000
EPS = 1e-5
_Q = dict(T=T, kv_dtype=1)
CELLS = (
    # q/k/v at 7B TP 1 / 8B / TP 4 / TP 8: cs 1 (int8: 12 streaming waves), 2, 4, 8 with the U fallbacks
    (QKV, 4096, 4, dict(hq=1, hkv=1, hd=64, **_Q)),
    (QKV, 4096, 8, dict(hq=1, hkv=1, hd=64, **_Q)),
    (QKV, 4096, 16, dict(hq=1, hkv=1, hd=64, **_Q)),
    (QKV, 4096, 31, dict(hq=1, hkv=1, hd=64, **_Q)),
    # MHA and GQA at both head sizes (the kv-head index is not 0), a masked tail, one chunk per row
    (QKV, 2736, 8, dict(hq=4, hkv=2, hd=64, **_Q)),
    (QKV, 2720, 8, dict(hq=4, hkv=2, hd=64, **_Q)),
    (QKV, 4096, 12, dict(hq=2, hkv=2, hd=128, **_Q)),
    (QKV, 256, 12, dict(hq=4, hkv=1, hd=128, **_Q)),
    # gate/up: 2.69 units per wave (7B), 2.94 (int8 keeps 16 waves), 3 each (8B), the TP shards, waves with no item
    (GATE_UP, 4096, 2, dict(inter=86)),
    (GATE_UP, 4096, 2, dict(inter=94)),
    (GATE_UP, 4096, 2, dict(inter=96)),
    (GATE_UP, 4096, 2, dict(inter=22)),
    (GATE_UP, 4096, 2, dict(inter=11)),
    (GATE_UP, 4096, 2, dict(inter=8)),
    (GATE_UP, 4096, 2, dict(inter=86, np=2)),
    (GATE_UP, 2736, 2, dict(inter=94, np=4)),
    (GATE_UP, 2720, 2, dict(inter=23, np=2)),
    # wo, plain input: TP 1 / 4 / 8 widths; cs 4 with every part real, and cs 4 of 5 (or 9) chunks: a part wholly past
    # the row end; 1100 units in one workgroup (the epilogue's non-prefetched path)
    (WO, 4096, 2, dict(nrows=32)),
    (WO, 1024, 2, dict(nrows=32)),
    (WO, 512, 2, dict(nrows=32)),
    (WO, 4096, 2, dict(nrows=12)),
    (WO, 4608, 2, dict(nrows=12)),
    (WO, 9216, 2, dict(nrows=12)),
    (WO, 64, 1, dict(nrows=1100)),
    # wo, merged input: NS 8 (max_splits 3, 8) and NS 16 (9, 16: the from-memory tail), hd 64 and 128, an input wider
    # than 4096 columns (merge_mem)
    (WO, 4096, 2, dict(nrows=32, merged=True, hq=32, hd=128, max_splits=8, ppwg=PPWG)),
    (WO, 1024, 2, dict(nrows=32, merged=True, hq=8, hd=128, max_splits=3, ppwg=PPWG)),
    (WO, 512, 2, dict(nrows=32, merged=True, hq=4, hd=128, max_splits=8, ppwg=PPWG)),
    (WO, 512, 2, dict(nrows=32, merged=True, hq=8, hd=64, max_splits=9, ppwg=PPWG)),
    (WO, 4096, 2, dict(nrows=33, merged=True, hq=64, hd=64, max_splits=16, ppwg=PPWG)),
    (WO, 5120, 2, dict(nrows=33, merged=True, hq=40, hd=128, max_splits=16, ppwg=PPWG)),
    # K-split wo: ks 2 and 4, hd 64 and 128, both NS
    (WO, 4096, 2, dict(nrows=32, hq=32, hd=128, max_splits=8, ppwg=PPWG, ks=2)),
    (WO, 4096, 4, dict(nrows=36, hq=64, hd=64, max_splits=9, ppwg=PPWG, ks=4)),
    (WO, 1024, 4, dict(nrows=30, hq=8, hd=128, max_splits=3, ppwg=PPWG, ks=2)),
    # down: 7B TP 1 / 4 / 8 and 8B widths (three chunks, masked), the K-split residual
    (DOWN, 11008, 2, dict(nrows=32)),
    (DOWN, 14336, 2, dict(nrows=32)),
    (DOWN, 2752, 2, dict(nrows=32)),
    (DOWN, 1376, 2, dict(nrows=32)),
    (DOWN, 11008, 2, dict(nrows=32, np=2)),
    (DOWN, 1376, 3, dict(nrows=70, np=4)),
    # LM head: odd row counts (the clamped second row of the last unit)
    (LOGITS, 4096, 2, dict(nrows=249)),
    (LOGITS, 4096, 2, dict(nrows=61)),
    (LOGITS, 4096, 2, dict(nrows=31)),
    (LOGITS, 4096, 2, dict(nrows=29)),
    (LOGITS, 256, 3, dict(nrows=61)),
)
ROLE_NAMES = {QKV: "qkv", GATE_UP: "gate_up", WO: "wo", DOWN: "down", LOGITS: "logits"}


def cell_takes(cell, wt):
    """Whether the weight type's vector divides the cell's columns (and, K-split, its column blocks)."""
    cols = cell[1] // cell[3].get("ks", 1)
    return cols % EPV[wt] == 0


def cell_id(cell):
    role, cols, cus, shape = cell
    return f"{ROLE_NAMES[role]}-{cols}-cus{cus}-" + "-".join(f"{k}{v}" for k, v in sorted(shape.items())
                                                              if k not in ("T", "kv_dtype", "ppwg"))


def merge_positions(max_splits):
    """Positions of a merged-input cell: 0, ppwg - 1, ppwg, 8 ppwg - 1, 8 ppwg and T - 1 for T = max_splits ppwg."""
    Tm = max_splits * PPWG
    return sorted({p for p in (0, PPWG - 1, PPWG, 8 * PPWG - 1, 8 * PPWG, Tm - 1) if p < Tm})
