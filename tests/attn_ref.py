"""float64 numpy restatement of ONE decode attention launch (simplellminference_amd/csrc/attention.h, attn_mfma.h), the
input builders, the error bound and the list of cells that tests/test_gpu_decode_attn.py holds the kernels to through
sli_decode_attn (include/sli.h "decode stages, for tests and labs"). test_attn_ref_cpu.py checks the arithmetic against
the C oracle and test_attn_stage_cpu.py the cell list against the geometries a production model runs.

The launch, for B sequences of hq query heads over hkv kv heads (g = hq / hkv) and a head-major cache [B hkv][T][hd]:
  s_t  = (q . k_t) / sqrt(hd) for t <= pos[b]              (fp32 fma chain, times the fp32 scale)
  out  = sum_t e^(s_t - M) v_t / sum_t e^(s_t - M)          (M = max s_t)
computed per split of ppwg positions as (o, m, l) = (sum e^(s_t - m) v_t, max s_t, sum e^(s_t - m)) and merged in split
order: a partial is compared in the normalisation-free form o / l and m + log l, which no choice of m changes.

Reused as they are: prefill_ref.attn, gemv_ref.merge / live_splits, kv8_ref (the FP8 table).
"""
from __future__ import annotations

import numpy as np

from tests import gemv_ref as G
from tests import kv8_ref as F8
from tests import prefill_ref as P

EPS32, U32 = P.EPS32, P.U32
DT = {"f32": 0, "f16": 1, "f8": 4}
POS_STRIDE = 6           # int32s between the sequences' positions (the engine's are kPosStride apart)
POS_POISON = 0x3FFFFFF0  # between them: a position read from there would be far outside every cache


# ---------------------------------------------------------------- the cache's exact values
def f8_encode(x):
    """kv8_ref.encode for fp32 input, in the integer arithmetic of sli.h's rule (sli_quant_f8): NaN -> 0x7F, |v| clamped
    to 448, below 2^-6 the step 2^-9 rounded by an fp32 add of 2^14, from 2^-6 up the fp32 word rounded to nearest even
    at its 20th bit and re-biased. Forty times faster than the table search; test_attn_ref_cpu.py holds the two equal."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    sign = ((u >> 24) & 0x80).astype(np.uint8)
    a = np.minimum(u & 0x7FFFFFFF, 0x43E00000).astype(np.uint32)
    t = (a.view(np.float32) + np.float32(16384.0)).view(np.uint32) - np.uint32(0x46800000)
    r = ((a + np.uint32(0x7FFFF) + ((a >> 20) & 1)) >> 20) - np.uint32(960)
    code = np.where(a < 0x3C800000, t, r).astype(np.uint8) | sign
    code[(u & 0x7FFFFFFF) > 0x7F800000] = 0x7F
    return code


def to_cache(x, kv):
    """x rounded to the cache type, as the device takes it (fp32 / fp16 arrays, uint8 E4M3 codes)."""
    if kv == "f8":
        return f8_encode(x)
    return np.asarray(x, np.float32).astype(np.float16 if kv == "f16" else np.float32)


def values(c, kv):
    """float64 of what the cache holds."""
    return F8.decode(c).astype(np.float64) if kv == "f8" else np.asarray(c, np.float64)


# ---------------------------------------------------------------- the reference
def decode(q, K, V, pos, hq, hkv, hd):
    """out [B hq hd] float64: per sequence b and q head h, softmax of (q . k_t) / sqrt(hd) over t <= pos[b] of kv head
    b hkv + h / (hq / hkv). q [B hq hd], K / V [B hkv][T][hd] (values), pos [B]."""
    B = len(pos)
    q = np.asarray(q, np.float64).reshape(B, hq * hd)
    return np.concatenate([P.attn(q[b:b + 1], K[b * hkv:(b + 1) * hkv], V[b * hkv:(b + 1) * hkv], int(pos[b]), hq, hkv,
                                  hd)[0] for b in range(B)])


def scores(q, K, pos, hq, hkv, hd):
    """Per (sequence, head): the float64 scores over t <= pos[b], as a list of [pos[b] + 1] arrays, [B hq]."""
    g = hq // hkv
    q = np.asarray(q, np.float64).reshape(len(pos) * hq, hd)
    return [K[(h // hq) * hkv + (h % hq) // g, :int(pos[h // hq]) + 1] @ q[h] / np.sqrt(hd) for h in range(len(q))]


def split_state(q, K, V, pos, hq, hkv, hd, ppwg, s):
    """Split s (rows [s ppwg, (s + 1) ppwg) up to pos[b]) of every head: (max score [H], log-sum-exp [H], o / l [H][hd])
    in float64; NaN for a head whose sequence does not reach the split."""
    g = hq // hkv
    H = len(pos) * hq
    q = np.asarray(q, np.float64).reshape(H, hd)
    m, lse, on = np.full(H, np.nan), np.full(H, np.nan), np.full((H, hd), np.nan)
    for h in range(H):
        b, p = h // hq, int(pos[h // hq])
        lo, hi = s * ppwg, min((s + 1) * ppwg, p + 1)
        if lo > p:
            continue
        kvh = b * hkv + (h % hq) // g
        sc = K[kvh, lo:hi] @ q[h] / np.sqrt(hd)
        m[h] = sc.max()
        w = np.exp(sc - m[h])
        lse[h] = m[h] + np.log(w.sum())
        on[h] = (w / w.sum()) @ V[kvh, lo:hi]
    return m, lse, on


def part_of_states(states, hd, max_splits):
    """part [H][max_splits][hd + 4] (o, m, l, pad) in float64 from split_state results, with l = 1 (o = o / l, m = the
    log-sum-exp): what gemv_ref.merge takes."""
    H = states[0][0].size
    part = np.full((H, max_splits, hd + 4), np.nan)
    for s, (_, lse, on) in enumerate(states):
        part[:, s, :hd], part[:, s, hd], part[:, s, hd + 1] = on, lse, 1.0
    return part


def merge_heads(part, ns_of_head, hd):
    """gemv_ref.merge head by head (each head has its own live split count): [H hd] float64."""
    return np.concatenate([G.merge(part[h:h + 1], int(ns_of_head[h]), hd)[0] for h in range(part.shape[0])])


# ---------------------------------------------------------------- the bound of the realistic family
def real_tol(q, K, V, pos, hq, hkv, hd, ns, split=None):
    """|out32 - out| per element for a kernel that computes the launch in fp32 from the cache's exact values.
    Scores: an fp32 fma chain of hd products (the register-staged kernels) or exact fp16 products summed in fp32 (MFMA:
    q travels as hi + mid + lo, 2^-33 relative) is within 4 eps32 sqrt(hd) sum_j |q_j k_tj| of the exact sum
    (gemv_ref.sum_tol), and the product with the fp32 scale adds two roundings of |s_t|:
        ds_t = (4 eps32 sqrt(hd) sum_j |q_j k_tj|) / sqrt(hd) + 2 u |s_t|.
    Through the softmax, to first order d out = sum_t p_t ds_t (v_t - out): |d out_d| <= max_t ds_t (A_d + |out_d|),
    A_d = sum_t p_t |v_td|, and max_t ds_t over the rows that carry weight (p_t >= 2^-40; the others' whole
    contribution is below 2^-40 A and is added as such) - doubled for the second order.
    The weights: s_t - m is rounded (u |s_t - m|, at most three times: the wave's m, the workgroup's, the merge's), expf
    is within 2 ulp (4 u) at each of the three levels, so the weight of row t carries (12 + 3 |s_t - M|) u relative:
    weighted, S = sum_t p_t |s_t - M|. The MFMA kernel passes p as fp16 hi + mid + lo: 2^-33 relative, or 2^-24
    absolute below 2^-9 (am_split3) - a row with p < 2^-9 contributes at most 2^-24 |v| instead of p |v|: 2^-24 sum_t
    |v_td| / L absolute, L >= 1 being the kernel's own normaliser (the row of the maximum has p = 1).
    The sums: o and l are sums of positive-weighted terms in chains of at most 16 per lane, 6 reduction steps, 16 waves
    and ns splits, one fma each: (40 + ns) u (A_d, resp. 1). The division: u.
    split = (ppwg, s): the same for the rows of split s alone (a partial in its o / l form; NaN for a head that does
    not reach it). Returns (tol [H hd], tol_lse [H]): m + log l carries the score error and the relative error of l."""
    H = len(pos) * hq
    g = hq // hkv
    qf = np.asarray(q, np.float64).reshape(H, hd)
    tol, tol_lse = np.full((H, hd), np.nan), np.full(H, np.nan)
    for h in range(H):
        b, p = h // hq, int(pos[h // hq])
        kvh = b * hkv + (h % hq) // g
        lo, hi = (0, p + 1) if split is None else (split[1] * split[0], min((split[1] + 1) * split[0], p + 1))
        if lo > p:
            continue
        Kl, Vl = K[kvh, lo:hi], V[kvh, lo:hi]
        s = Kl @ qf[h] / np.sqrt(hd)
        ds = 4 * EPS32 * (np.abs(Kl) @ np.abs(qf[h])) + 2 * U32 * np.abs(s)
        w = np.exp(s - s.max())
        pt = w / w.sum()
        heavy = pt >= 2.0 ** -40
        A = pt @ np.abs(Vl)
        o = pt @ Vl
        S = float(pt @ np.abs(s - s.max()))
        rel = 2 * float(ds[heavy].max()) + U32 * (12 + 3 * S + 40 + int(ns[h]) + 1) + 2.0 ** -40
        tol[h] = rel * (A + np.abs(o)) + 2.0 ** -24 * np.abs(Vl).sum(axis=0) / w.sum()
        tol_lse[h] = rel + 2 * U32 * abs(s.max() + np.log(w.sum()))
    return tol.reshape(-1), tol_lse


RTOL, ATOL = 1e-5, 2e-6  # tests/test_gpu_ops.py::test_mha's bar, kept on the unscaled heads


# ---------------------------------------------------------------- geometry of a plan
def slice_rows(plan):
    """Rows a wave owns contiguously: ppwg / waves (register-staged), one 32-key tile (MFMA)."""
    return 32 if plan["kernel"] else plan["ppwg"] // plan["waves"]


def positions(plan, T):
    """The positions the issue lists, for a plan's geometry: 0, one slice minus 1 and one slice, 31, 32, ppwg - 1,
    ppwg, one inside the last split that leaves waves with unequal live tiles and a masked tail inside a tile, T - 1."""
    ppwg, sl = plan["ppwg"], plan["ppwg"] // plan["waves"]
    s0 = (plan["max_splits"] - 1) * ppwg
    span = min(ppwg, T - s0)
    odd = s0 + (span // 2 + 13 if span // 2 + 13 < span else span // 2)
    out = []
    for p in (T - 1, odd, ppwg, ppwg - 1, 0, 32, 31, sl, sl - 1):  # (the long ones first: the needle family's rows)
        if 0 <= p < T and p not in out:
            out.append(p)
    return out


def pos_sets(plan, T, B, n, special=False, start=0):
    """n position vectors [B], every sequence of a vector at a different position where the list allows, rotating
    through positions() from index `start`; special: the first vector is (T - 1, 0, T - 1, ...): a sequence at 0
    between two at T - 1."""
    ps = positions(plan, T)
    out = []
    for i in range(n):
        v = [ps[(start + i * B + b) % len(ps)] for b in range(B)]
        out.append(v)
    if special and B >= 3:
        out[0] = [T - 1, 0, T - 1] + [ps[(3 + b) % len(ps)] for b in range(B - 3)]
    return out


def n_sets(B):
    """Position vectors a cell runs per family: 5 launches at batch 1, 3 of a batch (12 positions)."""
    return 5 if B == 1 else 3


def cell_sets(c, plan, fam):
    """The position vectors a cell runs in family fam ("needle", "uniform", "real"). A batch: 3 vectors of B positions
    (all nine listed positions, the first vector with a sequence at 0 between two at T - 1). Batch 1: 5 launches per
    family, the needle family from the long positions (its rows need them), the uniform family from the other end of
    the list, so that the two together run every listed position (test_attn_stage_cpu.py asserts it). A 17-split cell
    adds a vector with 17 live splits (the merge's two passes), exactly 16, 1, and the first row of the 17th. The
    realistic family runs the first two vectors and that one."""
    B, T, n = c["B"], c["T"], n_sets(c["B"])
    start = max(len(positions(plan, T)) - n, 0) if B == 1 and fam == "uniform" else 0
    sets = pos_sets(plan, T, B, n, special=B >= 3, start=start)
    if c.get("splits17"):
        ppwg = plan["ppwg"]
        assert plan["max_splits"] == 17 and T == 17 * ppwg and B == 4
        sets.append([T - 1, 16 * ppwg - 1, ppwg - 1, 16 * ppwg])
    return sets[:2] + sets[n:] if fam == "real" else sets


def pos_array(pos):
    """The int32 array the launch reads: stride POS_STRIDE, poison between the entries."""
    a = np.full((len(pos) - 1) * POS_STRIDE + 1 + 3, POS_POISON, np.int32)
    a[:(len(pos) - 1) * POS_STRIDE + 1:POS_STRIDE] = pos
    return a


def ns_of_heads(pos, hq, plan):
    return np.repeat([G.live_splits(int(p), plan["ppwg"], plan["max_splits"]) for p in pos], hq)


# ---------------------------------------------------------------- input builders
POISON = {"f32": 3e38, "f16": 65504.0, "f8": 0x7E}  # rows past pos[b]; f8: the code of 448


def poison_rows(Kc, Vc, pos, hkv, kv, nan=False):
    """Rows past pos[b] of every kv head: +-poison alternating (nan: NaN; FP8: the NaN codes 0x7F / 0xFF)."""
    T = Kc.shape[1]
    for kvh in range(Kc.shape[0]):
        p = int(pos[kvh // hkv])
        if p + 1 >= T:
            continue
        n = T - p - 1
        if kv == "f8":
            fill = np.where((np.arange(n * Kc.shape[2]) % 2).reshape(n, -1) == 0, 0x7E, 0xFE).astype(np.uint8) | \
                np.uint8(1 if nan else 0)
        else:
            sign = np.where((np.arange(n * Kc.shape[2]) % 2).reshape(n, -1) == 0, 1.0, -1.0)
            fill = (sign * (np.nan if nan else POISON[kv])).astype(Kc.dtype)
        Kc[kvh, p + 1:] = fill
        Vc[kvh, p + 1:] = fill[::-1]
    return Kc, Vc


NEEDLE_CLASSES = ("row0", "pos", "slice_first", "slice_last", "tile_first", "tile_last", "split_first", "split_last")


def needle_rows(pos, plan):
    """{class: row} of the needle rows a sequence at pos can take: row 0, pos, and the first and last row of a wave
    slice, of a 32-key tile and of a split (the last such boundary at or below pos, not row 0 / pos themselves)."""
    out = {"row0": 0, "pos": pos}
    for name, n in (("slice", slice_rows(plan)), ("tile", 32), ("split", plan["ppwg"])):
        first = (pos // n) * n
        if 0 < first <= pos:
            out[name + "_first"] = first
            out[name + "_last"] = first - 1
    return out


def needle(pos, hq, hkv, hd, T, kv, plan, seed, hits):
    """The needle family. For every (sequence, q head) a needle row t* <= pos[b] and a dimension j distinct per head of
    the kv head: q = 64 e_j, K[t*][j] = 64, every other live K element 0; V random integers of [-15, 15] without 0
    (exact in every cache type). The needle scores 4096 / sqrt(hd) >= 362, every other row 0, so every other weight
    is expf(<= -362) = 0 exactly in fp32 and out = V[t*] bit for bit. hits: {class: count} over the cell, updated (the
    least-hit class a head can take is taken). Returns q, K, V (cache arrays) and the expected out [B hq hd] fp32."""
    r = np.random.default_rng(seed)
    B, g = len(pos), hq // hkv
    q = np.zeros((B * hq, hd), np.float32)
    K = np.zeros((B * hkv, T, hd), np.float32)
    V = r.integers(1, 16, (B * hkv, T, hd)) * r.choice([-1, 1], (B * hkv, T, hd))
    want = np.zeros((B * hq, hd), np.float32)
    for h in range(B * hq):
        b = h // hq
        kvh = b * hkv + (h % hq) // g
        rows = needle_rows(int(pos[b]), plan)
        cls = min(rows, key=lambda c: (hits.get(c, 0), NEEDLE_CLASSES.index(c)))
        hits[cls] = hits.get(cls, 0) + 1
        j = (7 * kvh + 13 * (h % g) + 5 * (seed % 11)) % hd
        taken = {int(np.argmax(q[h2])) for h2 in range(h - h % g, h) if q[h2].any()}
        while j in taken:
            j = (j + 1) % hd
        q[h, j] = 64.0
        K[kvh, rows[cls], j] = 64.0
        want[h] = V[kvh, rows[cls]]
    assert 4096 / np.sqrt(hd) >= 362
    Kc, Vc = poison_rows(to_cache(K, kv), to_cache(V, kv), pos, hkv, kv)
    for kvh in range(B * hkv):  # the builder's claim, on the cache's own values
        p = int(pos[kvh // hkv])
        assert np.array_equal(values(Vc[kvh, :p + 1], kv), V[kvh, :p + 1])
        assert np.array_equal(values(Kc[kvh, :p + 1], kv), K[kvh, :p + 1])
    return q.reshape(-1), Kc, Vc, want.reshape(-1)


def uniform(pos, hq, hkv, hd, T, kv, seed):
    """The uniform family: K = 0 (every score 0, every weight 1, l = pos + 1), V integers of [-15, 15], q normal. o =
    sum V is an integer below 2^24 in every partial sum. Returns q, K, V (cache arrays), V's values."""
    r = np.random.default_rng(seed)
    B = len(pos)
    q = r.standard_normal(B * hq * hd).astype(np.float32)
    V = r.integers(-15, 16, (B * hkv, T, hd)).astype(np.float32)
    assert 15 * T < 2 ** 24
    K = np.zeros((B * hkv, T, hd), np.float32)
    Kc, Vc = poison_rows(to_cache(K, kv), to_cache(V, kv), pos, hkv, kv)
    return q, Kc, Vc, V.astype(np.float64)


def realistic(pos, hq, hkv, hd, T, kv, plan, seed):
    """The realistic family: q, K, V normal, K and V rounded to the cache type. Every other head is scaled: q times 8,
    and q[0] = 64 against K[t][0] = -16 in split 0 and +16 in every later split, so that on those heads split 0 lies
    at least 120 below the maximum wherever a second split is live (asserted): the merge's weights underflow there, as
    they should, while a maximum taken from split 0 would overflow expf. Returns q, K, V (cache arrays), the mask of
    scaled heads [B hq]."""
    r = np.random.default_rng(seed)
    B = len(pos)
    q = r.standard_normal((B * hq, hd)).astype(np.float32)
    K = r.standard_normal((B * hkv, T, hd)).astype(np.float32)
    V = r.standard_normal((B * hkv, T, hd)).astype(np.float32)
    scaled = np.arange(B * hq) % 2 == 1
    q[scaled] *= 8
    q[scaled, 0] = 64.0
    K[:, :, 0] = 16.0
    K[:, :plan["ppwg"], 0] = -16.0
    Kc, Vc = to_cache(K, kv), to_cache(V, kv)
    Kv = values(Kc, kv)
    sc = scores(q, Kv, pos, hq, hkv, hd)
    for h in np.flatnonzero(scaled):
        if int(pos[h // hq]) >= plan["ppwg"]:
            assert sc[h][:plan["ppwg"]].max() <= sc[h].max() - 120, (h, sc[h][:plan["ppwg"]].max(), sc[h].max())
    Kc, Vc = poison_rows(Kc, Vc, pos, hkv, kv)
    return q.reshape(-1), Kc, Vc, scaled


# ---------------------------------------------------------------- production launches and the cells
MODELS = {name: m[1:4] for name, m in G.MODELS.items()}  # hq, hkv, hd
# (model, TP degree, batch): gemv_ref's batch-1 launches, and Llama-3-8B at batch 8
PRODUCTION = tuple((model, tp, 1) for model, tp in G.PRODUCTION) + (("llama3-8b", 1, 8),)
# positions per workgroup of the register-staged kernel (ops.hip attn_wg_positions): test_attn_stage_cpu.py holds the
# table to sli_decode_attn_plan
PPWG_CACHE = {("f32", 128): 128, ("f32", 64): 256, ("f16", 128): 256, ("f16", 64): 512}


def production_merge(kv, hd, T, B):
    """The merge a model asks for (engine.hip): a batch 2 (kDeferBatched); batch 1: an FP8 cache 0, otherwise 1 up to
    8 splits of the cache type's own split length and 0 past that (wo_merges)."""
    if B > 1:
        return 2
    if kv == "f8":
        return 0
    return 1 if -(-T // PPWG_CACHE[(kv, hd)]) <= 8 else 0


def production_launches():
    """(kv, B, hq, hkv, hd, T, merge) of the attention launch of every model of PRODUCTION (model, TP degree, batch),
    with each cache type at T 2048 and 4096."""
    out = []
    for model, tp, B in PRODUCTION:
        hq, hkv, hd = MODELS[model]
        for kv in ("f32", "f16", "f8"):
            for T in (2048, 4096):
                out.append((kv, B, hq // tp, hkv // tp, hd, T, production_merge(kv, hd, T, B)))
    return out


def plan_class(kv, hd, plan):
    """What a launch exercises: (kernel, cache type, hd, g as launched, kv_group, merge as it took effect, ring slots
    min(tpw, ring), ring refilled tpw > nbuf, more than 16 splits: the merge's two passes)."""
    return (plan["kernel"], kv, hd, plan["g"], plan["kv_group"], plan["merge"], plan["nbuf"], plan["tpw"] > plan["nbuf"],
            plan["max_splits"] > 16)


def _c(name, kv, B, hq, hkv, hd, T, merge, cus, **kw):
    return dict(name=name, kv=kv, B=B, hq=hq, hkv=hkv, hd=hd, T=T, merge=merge, cus=cus, **kw)


def _cells():
    out = []
    # R1 register-staged, batch 1, the merge left to the consumer: fp16 and fp32, hd 128 and 64, G 1 and 2, 4 splits
    # (G 2: the last one 8 rows short)
    for kv in ("f16", "f32"):
        for hd in (128, 64):
            for g in (1, 2):
                T = 4 * PPWG_CACHE[(kv, hd)] - (8 if g == 2 else 0)
                out.append(_c("R1", kv, 1, 4 * g, 4, hd, T, 1, 64, nan=(hd == 128)))
    # R2 register-staged fp16 GQA-4, merge 1: cus on both sides of 2 Hkv wg_splits = 16 (two GQA-2 groups, and the
    # unsplit GQA-4 kernel); GQA-8
    out.append(_c("R2", "f16", 1, 8, 2, 128, 1024, 1, 16))
    out.append(_c("R2", "f16", 1, 8, 2, 128, 1024, 1, 15))
    out.append(_c("R2", "f16", 1, 8, 2, 64, 2048, 1, 16))
    out.append(_c("R2", "f16", 1, 16, 2, 128, 1000, 1, 16))
    # R3 fp32 cache, a batch of 4, the merge launch: G 1, 2, 4 (as GQA-4 and as two GQA-2 groups), 8; 17 splits
    out.append(_c("R3", "f32", 4, 2, 2, 128, 17 * 128, 2, 256, splits17=True))
    out.append(_c("R3", "f32", 4, 4, 2, 64, 1016, 2, 64))
    out.append(_c("R3", "f32", 4, 8, 2, 128, 17 * 128, 2, 256, splits17=True))
    out.append(_c("R3", "f32", 4, 8, 2, 128, 512, 2, 64))
    out.append(_c("R3", "f32", 4, 8, 2, 128, 512, 2, 32))
    out.append(_c("R3", "f32", 4, 16, 2, 64, 520, 2, 64))
    # R4 fp32 cache, batch 1: the in-launch last-arriver merge against the merge launch (pairs, bit for bit); cus below
    # 2 Hkv wg_splits = 64, so that the merge launch's GQA-4 cell runs the unsplit kernel the in-launch merge runs
    for g in (1, 4):
        for T in (1024, 17 * 128):
            for merge in (0, 2):
                out.append(_c("R4", "f32", 1, 4 * g, 4, 128, T, merge, 63))
    # M1 / M2 MFMA, fp16 and FP8, a batch of 4 x 2 kv heads, a merge launch requested (it becomes the in-launch
    # merge): every instantiation (hd, G, ring slots): tiles per wave 1 (hd 128 only), 2, and 3 (the ring refilled); 4, 2 and 2 splits
    for kv, name in (("f16", "M1"), ("f8", "M2")):
        for hd in (128, 64):
            for g in (1, 2, 4, 8):
                for cus in ((256, 16, 11) if hd == 128 else (16, 11)):
                    T = 512 if g in (1, 4) else 504
                    out.append(_c(name, kv, 4, 2 * g, 2, hd, T, 2, cus, nan=(g == 4 and hd == 128)))
    # M3 batch 1, the in-launch merge, fp16: the new entry against ops.mha_strided at cus 0
    out.append(_c("M3", "f16", 1, 8, 2, 128, 1024, 0, 0))
    out.append(_c("M3", "f16", 1, 4, 4, 64, 1000, 0, 0))
    return tuple(out)


CELLS = _cells()


def cell_id(c):
    return f"{c['name']}-{c['kv']}-B{c['B']}-hq{c['hq']}-hkv{c['hkv']}-hd{c['hd']}-T{c['T']}-m{c['merge']}-cus{c['cus']}"
