"""The prefill kernels (simplellminference_amd/csrc/prefill.h) one launch at a time, through the kernel-level entry
points of sli.h ("prefill stages, for tests and labs"), against the float64 reference tests/prefill_ref.py (itself
checked against the C oracle by test_prefill_ref_cpu.py). The entries pick the GEMM tiling and the attention kernel
through the functions the engine uses, so every cell of the picker table is run here exactly as sli_model_prefill
would run it.

Bars (derivations in prefill_ref.py next to each bound):
  (a) sums on dyadic-grid inputs: every product and partial sum is exact in fp32 in any order, so the sums must equal
      the reference BIT FOR BIT; where an epilogue rounds, only its own fp32 operations are allowed for:
        RoPE at position > 0: fl(fl(a0 c) -+ fl(a1 s)), three roundings, < 1.5 eps32 (|a0||c| + |a1||s|);
        SwiGLU: expf (<= 2 ulp), 1 + e, the division, sg * up, (SiLU: g * sg): <= 4 eps32 relative, plus the hi/lo
        split of the result, 2^-22 relative (one fp16 subnormal step, 2^-24, where the result is that small);
        an fp16 cache store is the round-to-nearest of the fp32 value: between fp16(ref - tol) and fp16(ref + tol),
        i.e. the rounded reference or, next to a tie, its neighbour (never more than one fp16 ulp away).
  (c) sums on realistic inputs: 4 eps32 sqrt(K) (|W| @ (|hi| + |lo|)) against the float64 sum of the identical
      rounded operands (test_matmul_f32's bound), passed through the epilogue's derivative, plus the terms of (a).
  (d) norm + split: hi + lo within rtol 2e-6 + 2^-22, atol 1e-7 of float64 (test_rmsnorm's bar plus the split).
  (e) attention: hi + lo within rtol 1e-5, atol 2e-6 of float64 per query (test_mha's bar for the decode kernels).

Measured on an MI355X: every cell of (a) is bit-exact at every depth and (e) holds as stated, so no bar here was
widened. The first run found pf_split(a * b) one fp16 ulp off next to fp16 ties (about 1 in 10^4 SwiGLU activations
and MFMA attention outputs), fixed in prefill.h. Kernels built without the lo MFMAs, or with one DMA
piece of each stage 1 KiB off in the ring, fail (a) in all 24 cells at all five depths.
"""
import numpy as np
import pytest

from tests import prefill_ref as R

pytestmark = pytest.mark.gpu

MS = (32, 64, 128, 256)
DEPTHS = (64, 128, 192, 704, 1024)  # fp16: 1, 2, 3, 11, 16 stages; int8: half, 1, 1.5, 5.5, 8 stages
QKV = dict(hq=15, hkv=3, hd=64)     # N = 1344
QKV128 = dict(hq=6, hkv=2, hd=128)  # N = 1280
INTER = 576                         # N = 1152
N_RESID = 1168
SENT16, SENT32 = 0x7E5A, 0x7FC5A5A5  # NaN bit patterns no kernel result equals


def _t(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sentinel(torch, shape, f16):
    if f16:
        return torch.full(shape, SENT16, dtype=torch.int16, device="cuda").view(torch.float16)
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _is_sentinel(a):
    return _bits(a) == (SENT16 if a.dtype == np.float16 else SENT32)


def _worst(err, tol):
    i = np.unravel_index(np.argmax(err - tol), err.shape)
    return f"err {err[i]:.3e} > tol {tol[i]:.3e} at {tuple(int(x) for x in i)} ({int((err > tol).sum())} of {err.size})"


def _hold(fails, tag, got, ref, tol):
    """|got - ref| <= tol elementwise (tol 0: equality of values)."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    tol = np.broadcast_to(np.asarray(tol, np.float64), err.shape)
    bad = ~(err <= tol)  # (NaN fails)
    if bad.any():
        fails.append(f"{tag}: {_worst(np.where(np.isnan(err), np.inf, err), tol)}")


def _geometry(tl, N):
    bn = 16 * tl["AT"] * tl["WR"]
    return bn, -(-N // bn)


@pytest.fixture(scope="module")
def tables(gpu):
    """sin / cos tables [T][hd / 2] (device, and as numpy) for T = 528, per head_dim."""
    from simplellminference_amd import ops
    out = {}
    for hd in (64, 128):
        s, c = ops.rope_cache(hd, 528, 10000.0)
        out[hd] = (s, c, s.cpu().numpy(), c.cpu().numpy())
    return out


# ---------------------------------------------------------------- launch + check helpers
def _run_qkv(torch, tables, W, scale, hi, lo, geo, kv, p0, nv, T):
    """One q/k/v GEMM on a sentinel-filled cache of three layers' worth of memory, the middle one under test.
    Returns q, the three layers of K and V (numpy, cache dtype) and the tiling."""
    from simplellminference_amd import ops
    hq, hkv, hd = geo["hq"], geo["hkv"], geo["hd"]
    M = hi.shape[0]
    sin_d, cos_d, _, _ = tables[hd]
    q = _sentinel(torch, (M, hq * hd), False)
    kc = _sentinel(torch, (3, hkv, T, hd), kv == "f16")
    vc = _sentinel(torch, (3, hkv, T, hd), kv == "f16")
    tl = ops.prefill_gemm_qkv(_t(torch, W), _t(torch, hi), _t(torch, lo), q, kc[1], vc[1], sin_d[:T], cos_d[:T], hq,
                              hkv, hd, p0, nv, row_scale=_t(torch, scale))
    return q.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy(), tl


def _check_qkv(fails, tag, tables, out, Y, dY, scale, geo, p0, nv, T):
    """q, K, V of _run_qkv against the reference epilogue of the float64 sums Y, known to +- dY (None: exact sums,
    so V rows and the rows at position 0 must be equal and the rest within the RoPE's own roundings). Every cache
    element outside rows p0 .. p0 + nv - 1 (below T) of the layer under test is still the sentinel."""
    q, kc, vc, _ = out
    hq, hkv, hd = geo["hq"], geo["hkv"], geo["hd"]
    _, _, sin_t, cos_t = tables[hd]
    sin_t, cos_t = sin_t[:T], cos_t[:T]
    M = Y.shape[0]
    nq, nk = hq * hd, hkv * hd
    a = Y * (1.0 if scale is None else scale.astype(np.float64))
    da = None
    if dY is not None:
        da = dY * (1.0 if scale is None else scale.astype(np.float64))
        if scale is not None:
            da = da + R.U32 * np.abs(a)  # the row-scale multiply rounds
    pos = np.minimum(p0 + np.arange(M), T - 1)
    q_ref, k_ref, v_ref, stored = R.epi_qkv(Y, scale, sin_t, cos_t, p0, nv, T, hq, hkv, hd)
    tol_q = R.rope_tol(a[:, :nq], pos, sin_t, cos_t, hd, None if da is None else da[:, :nq])
    tol_k = R.rope_tol(a[:, nq:nq + nk], pos, sin_t, cos_t, hd, None if da is None else da[:, nq:nq + nk])
    tol_v = np.zeros((M, nk)) if da is None else da[:, nq + nk:]
    if da is None:  # sin 0 = 0, cos 0 = 1: the rotation at position 0 is exact
        tol_q[pos == 0] = 0.0
        tol_k[pos == 0] = 0.0
    _hold(fails, f"{tag} q", q, q_ref, tol_q)  # every chunk row, padding included
    rows = p0 + np.nonzero(stored)[0]
    for name, cache, ref, tol in (("k", kc, k_ref, tol_k.reshape(M, hkv, hd)), ("v", vc, v_ref, tol_v.reshape(M, hkv, hd))):
        got = cache[1][:, rows, :].transpose(1, 0, 2)  # [stored rows][hkv][hd]
        if cache.dtype == np.float16:
            ok = R.within_f16_rounding(got, ref[stored], tol[stored])
            if not ok.all():
                err = np.abs(got.astype(np.float64) - ref[stored])
                fails.append(f"{tag} {name} (fp16 cache): {int((~ok).sum())} of {ok.size} outside the rounding of "
                             f"ref +- tol, max |got - ref| {np.nanmax(np.where(ok, 0, err)):.3e}")
        else:
            _hold(fails, f"{tag} {name}", got, ref[stored], tol[stored])
        untouched = np.ones(cache.shape, bool)
        untouched[1][:, rows, :] = False
        if not _is_sentinel(cache)[untouched].all():
            w = np.argwhere(~_is_sentinel(cache) & untouched)
            fails.append(f"{tag} {name}: {len(w)} elements written outside rows {p0}..{p0 + nv - 1} of the layer, "
                         f"first at [layer, head, row, d] = {w[0].tolist()}")


def _run_swiglu(torch, W, scale, hi, lo, silu):
    from simplellminference_amd import ops
    M, inter = hi.shape[0], W.shape[0] // 2
    ahi = _sentinel(torch, (M, inter), True)
    alo = _sentinel(torch, (M, inter), True)
    tl = ops.prefill_gemm_gate_up(_t(torch, W), _t(torch, hi), _t(torch, lo), ahi, alo, act_mode=silu,
                                  row_scale=_t(torch, scale))
    return R.joined(ahi.cpu().numpy(), alo.cpu().numpy()), tl


def _check_swiglu(fails, tag, got, Y, dY, scale, silu):
    inter = Y.shape[1] // 2
    sc = 1.0 if scale is None else scale.astype(np.float64)
    a = Y * sc
    g, u = a[:, :inter], a[:, inter:]
    dg = du = None
    if dY is not None:
        da = dY * sc + (R.U32 * np.abs(a) if scale is not None else 0.0)
        dg, du = da[:, :inter], da[:, inter:]
    _hold(fails, tag, got, R.act(g, u, silu), R.act_tol(g, u, silu, dg, du))


def _run_resid(torch, W, scale, hi, lo, resid, pad=0):
    """y [M][N + pad], sentinel-filled: the columns past N stay untouched."""
    from simplellminference_amd import ops
    M, N = hi.shape[0], W.shape[0]
    y = _sentinel(torch, (M, N + pad), False)
    tl = ops.prefill_gemm_resid(_t(torch, W), _t(torch, hi), _t(torch, lo), y, resid=_t(torch, resid),
                                row_scale=_t(torch, scale))
    y = y.cpu().numpy()
    assert _is_sentinel(y[:, N:]).all(), "columns past N were written"
    return y[:, :N], tl


# ---------------------------------------------------------------- (a) exact sums, every cell of the picker
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("role", [0, 1, 2])
@pytest.mark.parametrize("w", ["f16", "i8"])
def test_grid_sums_exact_every_picker_cell(gpu, tables, w, role, M):
    """One cell of the picker table (weight type, role, chunk size) at the five depths, on grid inputs (exact
    sums; hi and lo independent draws). role 2: y == resid + sum * scale bit for bit, with an integer-grid resid and
    with none (there into a wider y); role 0 (hd 64 GQA-5 at every depth, both cache types; one hd 128 shape): V
    rows and the q / k rows at position 0 equal, the rest within the RoPE's roundings, fp16 stores within the
    rounding of that; role 1 (sigmoid and SiLU): within the activation's roundings. The shapes give more than 8 row
    blocks, a count that is no multiple of 8 and (roles 0, 2) a partial last block; checked from the tiling the
    call reports."""
    torch = gpu
    int8 = w == "i8"
    fails, geom = [], []
    for K in DEPTHS:
        seed = 1000 * K + 10 * M + role
        if role == 2:
            N = N_RESID
            W, scale, hi, lo = R.grid_inputs(N, K, M, int8, seed)
            Y = R.gemm_sums(W, hi, lo)
            resid = R.grid_resid(M, N, seed + 1)
            y, tl = _run_resid(torch, W, scale, hi, lo, resid)
            _hold(fails, f"K {K} resid", y, R.epi_resid(Y, scale, resid), 0.0)
            y, tl2 = _run_resid(torch, W, scale, hi, lo, None, pad=16)
            _hold(fails, f"K {K} no resid", y, R.epi_resid(Y, scale, None), 0.0)
            assert tl2 == tl
        elif role == 1:
            N = 2 * INTER
            W, scale, hi, lo = R.grid_inputs(N, K, M, int8, seed)
            Y = R.gemm_sums(W, hi, lo)
            for silu in (0, 1):
                got, tl = _run_swiglu(torch, W, scale, hi, lo, silu)
                _check_swiglu(fails, f"K {K} silu {silu}", got, Y, None, scale, silu)
        else:
            shapes = [(QKV, "f32"), (QKV, "f16")] + ([(QKV128, "f32"), (QKV128, "f16")] if K == 192 else [])
            Y = None
            for geo, kv in shapes:
                N = (geo["hq"] + 2 * geo["hkv"]) * geo["hd"]
                if Y is None or Y.shape[1] != N:
                    W, scale, hi, lo = R.grid_inputs(N, K, M, int8, seed + N)
                    Y = R.gemm_sums(W, hi, lo)
                T = M + 8
                out = _run_qkv(torch, tables, W, scale, hi, lo, geo, kv, 0, M, T)
                _check_qkv(fails, f"K {K} hd {geo['hd']} kv {kv}", tables, out, Y, None, scale, geo, 0, M, T)
                if geo is QKV:
                    tl = out[3]
            N = 1344
        assert R.grid_units(W, hi, lo) < 2 ** 24
        bn, nrb = _geometry(tl, N)
        geom.append(nrb > 8 and nrb % 8 != 0 and (N % bn != 0 or not ((role in (0, 2) and bn == 128) or N == N_RESID)))
        ks = 128 if int8 else 64
        if K == DEPTHS[-1]:
            assert -(-K // ks) > max(tl["S"], tl["SA"]), "the deepest case must wrap every ring"
    assert tl["BM"] <= M and M % tl["BM"] == 0 and tl["PIPE"] in (0, 1)
    assert any(geom), f"no depth met the row-block conditions: tiling {tl}"
    assert not fails, f"tiling {tl}:\n" + "\n".join(fails)


def test_picker_table_has_a_split_ring_cell(gpu, tables):
    """The table's one split-ring tiling (SA > 0, the weights in a ring of their own) is among the cells above; if a
    later table drops or moves it this says so, so the depths above keep covering its prologue guards."""
    torch = gpu
    tilings = {}
    for w in ("f16", "i8"):
        for M in MS:
            W, scale, hi, lo = R.grid_inputs(1024, 64, M, w == "i8", 1)
            tilings[(w, 2, M)] = _run_resid(torch, W, scale, hi, lo, None)[1]
            tilings[(w, 1, M)] = _run_swiglu(torch, W, scale, hi, lo, 0)[1]
            geo = dict(hq=8, hkv=4, hd=64)
            tilings[(w, 0, M)] = _run_qkv(torch, tables, W, scale, hi, lo, geo, "f16", 0, M, M)[3]
    assert len(tilings) == 24
    split = {c: t for c, t in tilings.items() if t["SA"] > 0}
    assert split, "no cell of the picker table runs the split weight ring"
    for c, t in split.items():
        assert t["SA"] > t["S"] and t["PIPE"] == 1, (c, t)  # prefill.h: SA == S computed wrong sums
        assert 1024 // 64 > 2 * t["SA"], (c, t)  # the deepest case of the test above wraps this ring more than once


@pytest.mark.parametrize("K", [64, 192, 704])
@pytest.mark.parametrize("w", ["f16", "i8"])
def test_reads_stay_inside_weights_scales_and_activations(gpu, w, K):
    """The weights, the int8 row scales and the hi / lo activations are views into larger buffers filled in front and
    behind with a value that changes any sum it enters (NaN; int8: 127): a DMA piece that ran past a row's end,
    multiplied in, would show. The depths are 64 mod 128, so int8 ends in a half stage whose pieces step back (1, 3
    and 11 fp16 stages). Exact grid sums, and the guard regions stay as they were."""
    torch = gpu
    from simplellminference_amd import ops
    N, M, guard = N_RESID, 32, 4096
    W, scale, hi, lo = R.grid_inputs(N, K, M, w == "i8", 700 + K)
    Y = R.epi_resid(R.gemm_sums(W, hi, lo), scale, None)
    bufs = []

    def view(a):
        if a is None:
            return None
        t = _t(torch, a)
        big = torch.full((guard + t.numel() + guard,), 127 if t.dtype == torch.int8 else float("nan"), dtype=t.dtype,
                         device="cuda")
        v = big[guard:guard + t.numel()].view(t.shape)
        v.copy_(t)
        bufs.append(big)
        return v

    y = _sentinel(torch, (M, N), False)
    ops.prefill_gemm_resid(view(W), view(hi), view(lo), y, resid=None, row_scale=view(scale))
    fails = []
    _hold(fails, f"{w} K {K} views", y.cpu().numpy(), Y, 0.0)
    assert not fails, "\n".join(fails)
    assert len(bufs) == (4 if w == "i8" else 3)
    for big in bufs:
        for g in (big[:guard], big[-guard:]):
            assert bool(((g == 127) if big.dtype == torch.int8 else g.isnan()).all())


# ---------------------------------------------------------------- (b) padding and bounds of the cache stores
def _bounds_cases(M):
    return [(0, M - 27, M + 8), (256, M, 256 + M + 8), (256, M - 20, 256 + M - 20), (256, M, 256 + M - 20)]


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("M", [64, 256])
@pytest.mark.parametrize("kv", ["f16", "f32"])
def test_qkv_cache_stores_stay_in_their_rows(gpu, tables, kv, M, case):
    """(p0, nv, T): fewer valid rows than chunk rows; a chunk starting at 256; the last valid row at T - 1 with the
    padding rows past T; and every row valid by count with the last 20 past T (only the pos < T guard keeps them out
    of the next head's rows). The cache holds a NaN sentinel; afterwards exactly rows p0 .. p0 + nv - 1 (below T) of
    every kv head of the layer under test hold the reference's values, and every other element, the layers in front
    and behind included, is bitwise the sentinel. q is there for all M rows (RoPE at the clamped position)."""
    torch = gpu
    p0, nv, T = _bounds_cases(M)[case]
    fails = []
    N = (QKV["hq"] + 2 * QKV["hkv"]) * QKV["hd"]
    W, scale, hi, lo = R.grid_inputs(N, 128, M, False, 7 + case)
    Y = R.gemm_sums(W, hi, lo)
    out = _run_qkv(torch, tables, W, scale, hi, lo, QKV, kv, p0, nv, T)
    _check_qkv(fails, f"p0 {p0} nv {nv} T {T}", tables, out, Y, None, scale, QKV, p0, nv, T)
    kc = out[1]
    written = ~_is_sentinel(kc)[1].all(axis=(0, 2))  # rows of the layer with anything written
    assert np.array_equal(np.nonzero(written)[0], np.arange(p0, min(p0 + nv, T))), np.nonzero(written)[0]
    assert not np.isnan(out[0]).any()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- (c) realistic values
def _real_weights(oracle, N, K, int8, seed):
    r = np.random.default_rng(seed)
    w = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    if not int8:
        return w.astype(np.float16), None
    q = np.empty((N, K), np.int8)
    s = np.empty(N, np.float32)
    for i in range(N):
        q[i], s[i] = oracle.quant_row_i8(w[i])
    return q, s


def _real_acts(torch, M, K, seed):
    """standard_normal activations split by the kernel under test itself; the reference takes the same hi, lo."""
    from simplellminference_amd import ops
    x = np.random.default_rng(seed).standard_normal((M, K)).astype(np.float32)
    hi, lo = ops.prefill_norm_split(_t(torch, x), None, 1e-5)
    return hi.cpu().numpy(), lo.cpu().numpy()


@pytest.mark.parametrize("M", [64, 256])
@pytest.mark.parametrize("role", [0, 1, 2])
@pytest.mark.parametrize("w", ["f16", "i8"])
def test_realistic_values(gpu, oracle, tables, w, role, M):
    """K = 704, N(0, 1) activations, N(0, 1/K) weights (int8: oracle.quant_row_i8 rows and scales). The sum is held
    to 4 eps32 sqrt(K) (|W| @ (|hi| + |lo|)) around the float64 sum of the same rounded operands; the epilogues add
    their own terms (module docstring)."""
    torch = gpu
    K, int8, fails = 704, w == "i8", []
    N = {0: 1344, 1: 2 * INTER, 2: N_RESID}[role]
    W, scale = _real_weights(oracle, N, K, int8, 11 * M + role)
    hi, lo = _real_acts(torch, M, K, 5 * M + role)
    Y = R.gemm_sums(W, hi, lo)
    dY = 4 * R.EPS32 * np.sqrt(K) * R.gemm_abs(W, hi, lo)
    if role == 2:
        _check_resid_real(fails, torch, W, scale, hi, lo, Y, dY, M)
    elif role == 1:
        for silu in (0, 1):
            got, _ = _run_swiglu(torch, W, scale, hi, lo, silu)
            _check_swiglu(fails, f"silu {silu}", got, Y, dY, scale, silu)
    else:
        p0, T = 5, M + 16
        for kv in ("f16", "f32"):
            out = _run_qkv(torch, tables, W, scale, hi, lo, QKV, kv, p0, M, T)
            _check_qkv(fails, f"kv {kv}", tables, out, Y, dY, scale, QKV, p0, M, T)
    assert not fails, "\n".join(fails)


def _check_resid_real(fails, torch, W, scale, hi, lo, Y, dY, M):
    """y = resid + sum * scale: the sum's bound times the scale, the scale multiply (u |p|) and the add (u |y|)."""
    N = W.shape[0]
    sc = 1.0 if scale is None else scale.astype(np.float64)
    for resid in (np.random.default_rng(M).standard_normal((M, N)).astype(np.float32), None):
        y, _ = _run_resid(torch, W, scale, hi, lo, resid)
        ref = R.epi_resid(Y, scale, resid)
        tol = dY * sc + R.EPS32 * (np.abs(Y * sc) + (0.0 if resid is None else np.abs(resid)))
        _hold(fails, f"resid {resid is not None}", y, ref, tol)


@pytest.mark.parametrize("w", ["f16", "i8"])
def test_realistic_values_deep(gpu, oracle, w):
    """K = 4096, N = 1168, M = 256, wo / down: 64 (int8: 32) stages, the depth of the 7B projections."""
    torch = gpu
    K, M, fails = 4096, 256, []
    W, scale = _real_weights(oracle, N_RESID, K, w == "i8", 3)
    hi, lo = _real_acts(torch, M, K, 4)
    Y = R.gemm_sums(W, hi, lo)
    dY = 4 * R.EPS32 * np.sqrt(K) * R.gemm_abs(W, hi, lo)
    _check_resid_real(fails, torch, W, scale, hi, lo, Y, dY, M)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- (d) norm and split
@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("D", [64, 320, 4096, 8192])
def test_norm_split(gpu, D, weights):
    """32 rows of RMSNorm + split (without weights: the plain split of x, which must then be exact): hi + lo against
    float64 at test_rmsnorm's bar plus the split's 2^-22, and |lo| <= 2^-11 |hi|: a proper split."""
    torch = gpu
    from simplellminference_amd import ops
    r = np.random.default_rng(D + weights)
    x = r.standard_normal((32, D)).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(D)).astype(np.float32) if weights else None
    hi, lo = ops.prefill_norm_split(_t(torch, x), _t(torch, w), 1e-5)
    hi, lo = hi.cpu().numpy(), lo.cpu().numpy()
    ref = R.norm(x, w, 1e-5)
    err = np.abs(R.joined(hi, lo) - ref)
    lim = 1e-7 + (2e-6 + R.SPLIT_REL) * np.abs(ref)
    assert np.all(err <= lim), _worst(err, lim)
    assert np.all(np.abs(lo.astype(np.float64)) <= 2.0 ** -11 * np.abs(hi.astype(np.float64)))
    if not weights:
        whi, wlo = R.split(x)
        assert np.array_equal(_bits(hi), _bits(whi)) and np.array_equal(lo.astype(np.float64), wlo.astype(np.float64))


# ---------------------------------------------------------------- (e) attention, per query
POSITIONS = [(0, 64, 64), (256, 64, 320), (256, 64, 300), (0, 32, 64)]  # (p0, M, T)
ATTN = [("f16", hd, hq, hkv) for hd in (64, 128) for hq, hkv in ((2, 2), (8, 2))] + \
       [("f32", hd, 4, 2) for hd in (64, 128)]


@pytest.mark.parametrize("p0,M,T", POSITIONS)
@pytest.mark.parametrize("kv,hd,hq,hkv", ATTN)
def test_prefill_attention_per_query(gpu, kv, hd, hq, hkv, p0, M, T):
    """pf_attn_mfma_kernel (fp16 cache; MHA and GQA-4) and pf_attn_kernel (fp32 cache) against float64 attention per
    chunk row, at test_mha's bar. Positions: one or two 32-key tiles (three of the MFMA kernel's four waves have
    none); 9 to 10 tiles (every wave refills its image, four partial results merge); key tiles and query rows
    crossing T (rows below T - p0 compared); 32 chunk rows, where the fp32 kernel's 64-row block reads and writes
    rows 32 .. 63 of buffers that hold them (the contract of sli_prefill_attn)."""
    torch = gpu
    from simplellminference_amd import ops
    r = np.random.default_rng(p0 + M + T + hd + hq)
    rows = M if kv == "f16" else max(M, 64)
    q = r.standard_normal((rows, hq * hd)).astype(np.float32)
    K = r.standard_normal((hkv, T, hd)).astype(np.float32)
    V = r.standard_normal((hkv, T, hd)).astype(np.float32)
    if kv == "f16":
        K, V = K.astype(np.float16), V.astype(np.float16)
    ohi, olo = ops.prefill_attn(_t(torch, q), _t(torch, K), _t(torch, V), M, p0, hq, hkv, hd)
    got = R.joined(ohi.cpu().numpy(), olo.cpu().numpy())[:M]
    ref = R.attn(q, K, V, p0, hq, hkv, hd, rows=M)
    n = min(M, T - p0)
    assert n > 0 and not np.isnan(ref[:n]).any()
    err = np.abs(got[:n] - ref[:n])
    lim = 2e-6 + 1e-5 * np.abs(ref[:n])
    assert np.all(err <= lim), _worst(err, lim)


# ---------------------------------------------------------------- argument checks (nothing is launched)
def test_entry_points_reject_what_the_kernels_cannot_take(gpu):
    torch = gpu
    from simplellminference_amd import ops
    from simplellminference_amd._lib import SliError

    def rejected(fn, *a, **k):
        with pytest.raises(SliError) as e:
            fn(*a, **k)
        assert e.value.code == 1, e.value  # SLI_ERR_ARG

    def f16(*s):
        return torch.zeros(*s, dtype=torch.float16, device="cuda")

    def f32(*s):
        return torch.zeros(*s, dtype=torch.float32, device="cuda")

    rejected(ops.prefill_norm_split, f32(2, 6), None, 1e-5)      # D % 4
    rejected(ops.prefill_norm_split, f32(2, 8196), None, 1e-5)   # D > 8192
    rejected(ops.prefill_gemm_resid, f16(64, 64), f16(48, 64), f16(48, 64), f32(48, 64))    # M not a chunk size
    rejected(ops.prefill_gemm_resid, f16(64, 96), f16(32, 96), f16(32, 96), f32(32, 64))    # K % 64
    rejected(ops.prefill_gemm_resid, f16(24, 64), f16(32, 64), f16(32, 64), f32(32, 24))    # N % 16
    rejected(ops.prefill_gemm_resid, f16(64, 64), f16(32, 64), f16(32, 64), f32(32, 62))    # ld < N
    rejected(ops.prefill_gemm_gate_up, f16(64, 64), f16(32, 64), f16(32, 64), f16(32, 32), f16(32, 32), act_mode=2)
    s, c = f32(40, 48), f32(40, 48)
    rejected(ops.prefill_gemm_qkv, f16(4 * 96, 64), f16(32, 64), f16(32, 64), f32(32, 2 * 96), f16(1, 40, 96),
             f16(1, 40, 96), s, c, 2, 1, 96, 0, 32)              # hd 96
    s, c = f32(40, 32), f32(40, 32)
    rejected(ops.prefill_gemm_qkv, f16(7 * 64, 64), f16(32, 64), f16(32, 64), f32(32, 3 * 64), f16(2, 40, 64),
             f16(2, 40, 64), s, c, 3, 2, 64, 0, 32)              # hq no multiple of hkv
    rejected(ops.prefill_gemm_qkv, f16(4 * 64, 64), f16(32, 64), f16(32, 64), f32(32, 2 * 64), f16(1, 40, 64),
             f16(1, 40, 64), s, c, 2, 1, 64, 0, 33)              # nv > M
    rejected(ops.prefill_attn, f32(32, 128), f32(1, 64, 64), f32(1, 64, 64), 32, 0, 2, 1, 64)    # fp32: 64 rows needed
    rejected(ops.prefill_attn, f32(64, 192), f16(2, 64, 64), f16(2, 64, 64), 64, 0, 3, 2, 64)    # hq % hkv
    rejected(ops.prefill_attn, f32(64, 128), f16(1, 64, 64), f16(1, 64, 64), 64, 64, 2, 1, 64)   # p0 >= T
    rejected(ops.prefill_attn, f32(48, 128), f16(1, 64, 64), f16(1, 64, 64), 48, 0, 2, 1, 64)    # M not a chunk size
