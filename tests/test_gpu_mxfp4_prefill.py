"""Prompt prefill on MXFP4 weights: pgemm_kernel<…, mxfp4> (simplellminference_amd/csrc/prefill.h) one launch at a time
through sli_prefill_gemm_mxfp4, against the float64 reference of tests/prefill_ref.py on W = the rule's
dequantisation of the codes and scales (tests/mxfp4_ref.py), then the model path behind set_prefill("gemm") against an
eager fp32 oracle whose matrices were overwritten with that dequantisation.

Bars: those of tests/test_gpu_prefill_kernels.py (derivations there and in prefill_ref.py): on grid inputs
(tests/mxfp4_prefill_ref.py: every product and partial sum exact in fp32 in any order) the sums equal float64 BIT FOR
BIT and only an epilogue's own fp32 roundings are allowed for; on realistic inputs 4 eps32 sqrt(K) (|W| @ (|hi| +
|lo|)) around the float64 sum of the same operands plus the epilogue terms. Model level: the bars of
test_gpu_prefill.py (tokens equal, logits of computed positions within 1e-3, K/V rows within 2e-3).
"""
import ctypes

import numpy as np
import pytest

from tests import mxfp4_prefill_ref as G
from tests import mxfp4_ref as mx
from tests import prefill_ref as R

pytestmark = pytest.mark.gpu

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


@pytest.fixture(scope="module")
def tables(gpu):
    """sin / cos tables [T][hd / 2] (device, and as numpy) for T = 528, per head_dim."""
    from simplellminference_amd import ops
    out = {}
    for hd in (64, 128):
        s, c = ops.rope_cache(hd, 528, 10000.0)
        out[hd] = (s, c, s.cpu().numpy(), c.cpu().numpy())
    return out


class Wmx:
    """MXFP4 weights on the device (public layout) and as float64."""

    def __init__(self, torch, codes, scales):
        self.data, self.scales = _t(torch, mx.pack(codes)), _t(torch, scales)
        self.W = G.weights64(codes, scales)
        self.N = codes.shape[0]


# ---------------------------------------------------------------- launch + check helpers (scale-free restatements of
# test_gpu_prefill_kernels.py's: MXFP4 has no row scale)
def _run_qkv(torch, tables, w, hi, lo, geo, kv, p0, nv, T):
    from simplellminference_amd import ops
    hq, hkv, hd = geo["hq"], geo["hkv"], geo["hd"]
    M = hi.shape[0]
    sin_d, cos_d, _, _ = tables[hd]
    q = _sentinel(torch, (M, hq * hd), False)
    kc = _sentinel(torch, (3, hkv, T, hd), kv == "f16")
    vc = _sentinel(torch, (3, hkv, T, hd), kv == "f16")
    tl = ops.prefill_gemm_qkv(w.data, _t(torch, hi), _t(torch, lo), q, kc[1], vc[1], sin_d[:T], cos_d[:T], hq, hkv, hd,
                              p0, nv, scales=w.scales)
    return q.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy(), tl


def _check_qkv(fails, tag, tables, out, Y, dY, geo, p0, nv, T):
    """q, K, V against the reference epilogue of the float64 sums Y, known to +- dY (None: exact sums, so V rows and
    the rows at position 0 must be equal and the rest within the RoPE's own roundings). Every cache element outside
    rows p0 .. p0 + nv - 1 (below T) of the layer under test is still the sentinel."""
    q, kc, vc, _ = out
    hq, hkv, hd = geo["hq"], geo["hkv"], geo["hd"]
    _, _, sin_t, cos_t = tables[hd]
    sin_t, cos_t = sin_t[:T], cos_t[:T]
    M = Y.shape[0]
    nq, nk = hq * hd, hkv * hd
    pos = np.minimum(p0 + np.arange(M), T - 1)
    q_ref, k_ref, v_ref, stored = R.epi_qkv(Y, None, sin_t, cos_t, p0, nv, T, hq, hkv, hd)
    tol_q = R.rope_tol(Y[:, :nq], pos, sin_t, cos_t, hd, None if dY is None else dY[:, :nq])
    tol_k = R.rope_tol(Y[:, nq:nq + nk], pos, sin_t, cos_t, hd, None if dY is None else dY[:, nq:nq + nk])
    tol_v = np.zeros((M, nk)) if dY is None else dY[:, nq + nk:]
    if dY is None:  # sin 0 = 0, cos 0 = 1: the rotation at position 0 is exact
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


def _run_swiglu(torch, w, hi, lo, silu):
    from simplellminference_amd import ops
    M, inter = hi.shape[0], w.N // 2
    ahi = _sentinel(torch, (M, inter), True)
    alo = _sentinel(torch, (M, inter), True)
    tl = ops.prefill_gemm_gate_up(w.data, _t(torch, hi), _t(torch, lo), ahi, alo, act_mode=silu, scales=w.scales)
    return R.joined(ahi.cpu().numpy(), alo.cpu().numpy()), tl


def _check_swiglu(fails, tag, got, Y, dY, silu):
    inter = Y.shape[1] // 2
    g, u = Y[:, :inter], Y[:, inter:]
    dg, du = (None, None) if dY is None else (dY[:, :inter], dY[:, inter:])
    _hold(fails, tag, got, R.act(g, u, silu), R.act_tol(g, u, silu, dg, du))


def _run_resid(torch, w, hi, lo, resid, pad=0, data=None, scales=None, acts=None):
    """y [M][N + pad], sentinel-filled: the columns past N stay untouched. acts: device (hi, lo) to use instead."""
    from simplellminference_amd import ops
    M, N = hi.shape[0], w.N
    y = _sentinel(torch, (M, N + pad), False)
    dhi, dlo = (_t(torch, hi), _t(torch, lo)) if acts is None else acts
    tl = ops.prefill_gemm_resid(w.data if data is None else data, dhi, dlo, y,
                                resid=_t(torch, resid), scales=w.scales if scales is None else scales)
    y = y.cpu().numpy()
    assert _is_sentinel(y[:, N:]).all(), "columns past N were written"
    return y[:, :N], tl


# ---------------------------------------------------------------- 1. exact sums, every cell of the picker
@pytest.mark.parametrize("M", G.MS)
@pytest.mark.parametrize("role", [0, 1, 2])
def test_grid_sums_exact_every_picker_cell(gpu, tables, role, M):
    """One cell of pg_pick<mxfp4> (role, chunk size) at the six depths (128-k stages: half a stage, 1, 1.5, 2.5, 5.5
    and 16, the last wrapping every ring), uniform codes, block exponents from a 6-binade window (5 at K = 2048) around
    2^-7, hi and lo independent k / 8 draws. The bars of test_gpu_prefill_kernels.py's test of the same name."""
    torch = gpu
    fails = []
    cases = G.cell_cases(role, M)
    assert [c[1] for c in cases if c[0] != 1280] == list(G.DEPTHS)
    for N, K, seed in cases:
        codes, scales, hi, lo = G.grid_inputs(N, K, M, seed)
        assert G.grid_units(codes, scales, hi, lo) < 2 ** 24
        w = Wmx(torch, codes, scales)
        Y = R.gemm_sums(w.W, hi, lo)
        if role == 2:
            resid = R.grid_resid(M, N, seed + 1) * 2.0 ** (G.CENTRE - 7)  # on the sums' grid: resid + sum stays exact
            y, tl = _run_resid(torch, w, hi, lo, resid)
            _hold(fails, f"K {K} resid", y, R.epi_resid(Y, None, resid), 0.0)
            y, tl2 = _run_resid(torch, w, hi, lo, None, pad=16)
            _hold(fails, f"K {K} no resid", y, Y, 0.0)
            assert tl2 == tl
        elif role == 1:
            for silu in (0, 1):
                got, tl = _run_swiglu(torch, w, hi, lo, silu)
                _check_swiglu(fails, f"K {K} silu {silu}", got, Y, None, silu)
        else:
            geo = G.QKV if N == 1344 else G.QKV128
            T = M + 8
            for kv in ("f32", "f16"):
                out = _run_qkv(torch, tables, w, hi, lo, geo, kv, 0, M, T)
                _check_qkv(fails, f"K {K} hd {geo['hd']} kv {kv}", tables, out, Y, None, geo, 0, M, T)
            tl = out[3]
        bn = 16 * tl["AT"] * tl["WR"]
        nrb = -(-N // bn)
        if N != 1280:
            assert nrb > 8 and nrb % 8 != 0, (tl, N)  # more than one round of the 8 XCDs, a padded grid
        assert role != 2 or N % bn != 0, (tl, N)  # wo / down: a partial last row block
        assert tl["KS"] in (128, 256) and tl["BM"] <= M and M % tl["BM"] == 0
        if K == G.DEPTHS[-1]:
            assert -(-K // tl["KS"]) > max(tl["S"], tl["SA"]), "the deepest case must wrap every ring"
    assert not fails, f"tiling {tl}:\n" + "\n".join(fails)


# ---------------------------------------------------------------- 2. the whole scale range
def test_block_scales_far_outside_fp16(gpu):
    """Row r's exponent window is centred at 2^-100, -40, -17, 0, 12, 40, 100 by r % 7: a kernel that multiplies the
    scale into an fp16 operand overflows or flushes most rows. Bit-equal to float64."""
    torch = gpu
    N, K, M = G.N_RESID, 704, 64
    codes, scales, hi, lo = G.grid_inputs(N, K, M, 77, centres=G.range_centres(N))
    assert G.grid_units(codes, scales, hi, lo) < 2 ** 24
    w = Wmx(torch, codes, scales)
    Y = R.gemm_sums(w.W, hi, lo)
    assert np.array_equal(Y.astype(np.float32).astype(np.float64), Y) and np.abs(Y).max() > 2.0 ** 100
    y, _ = _run_resid(torch, w, hi, lo, None)
    fails = []
    _hold(fails, "scale range", y, Y, 0.0)
    assert not fails, "\n".join(fails) + f"\nrows off by centre: " + str(
        {c: int((y != Y)[:, G.range_centres(N) == c].sum()) for c in G.RANGE_CENTRES})


# ---------------------------------------------------------------- 3. reads stay inside the operands
@pytest.mark.parametrize("K", [64, 192, 704])
def test_reads_stay_inside_data_and_scales(gpu, K):
    """data and scales are views into larger buffers filled with 0xFF (scale byte 255, elements -6) in front and
    behind, the hi / lo activations views into buffers filled with NaN: a DMA piece of a short last stage that ran
    past a row's end, multiplied in, would change the sums. The scales view starts at an odd byte."""
    torch = gpu
    N, M = G.N_RESID, 32
    codes, scales, hi, lo = G.grid_inputs(N, K, M, 500 + K)
    w = Wmx(torch, codes, scales)
    Y = R.gemm_sums(w.W, hi, lo)
    big_d = torch.full((4096 + N * K // 2 + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    big_s = torch.full((4099 + N * K // 32 + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    dv = big_d[4096:4096 + N * K // 2].view(N, K // 2)
    sv = big_s[4099:4099 + N * K // 32].view(N, K // 32)
    dv.copy_(w.data)
    sv.copy_(w.scales)
    big_a = [torch.full((4096 + M * K + 4096,), float("nan"), dtype=torch.float16, device="cuda") for _ in range(2)]
    av = [b[4096:4096 + M * K].view(M, K) for b in big_a]
    av[0].copy_(_t(torch, hi))
    av[1].copy_(_t(torch, lo))
    y, _ = _run_resid(torch, w, hi, lo, None, data=dv, scales=sv, acts=av)
    fails = []
    _hold(fails, f"K {K} views", y, Y, 0.0)
    assert not fails, "\n".join(fails)
    assert bool((big_d[:4096] == 0xFF).all()) and bool((big_s[:4099] == 0xFF).all())
    assert bool((big_d[-4096:] == 0xFF).all()) and bool((big_s[-4096:] == 0xFF).all())
    for b in big_a:
        assert bool(b[:4096].isnan().all()) and bool(b[-4096:].isnan().all())


# ---------------------------------------------------------------- 4. realistic values
def _real_weights(torch, N, K, seed):
    """N(0, 1 / K) weights through the device quantiser; W is the rule's dequantisation of what it stored."""
    from simplellminference_amd import ops
    w32 = (np.random.default_rng(seed).standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    data, scales = ops.quant_mxfp4(_t(torch, w32))
    w = Wmx.__new__(Wmx)
    w.data, w.scales, w.N = data, scales, N
    w.W = G.weights64(mx.unpack(data.cpu().numpy()), scales.cpu().numpy())
    return w


def _real_acts(torch, M, K, seed):
    from simplellminference_amd import ops
    x = np.random.default_rng(seed).standard_normal((M, K)).astype(np.float32)
    hi, lo = ops.prefill_norm_split(_t(torch, x), None, 1e-5)
    return hi.cpu().numpy(), lo.cpu().numpy()


def _check_resid_real(fails, torch, w, hi, lo, Y, dY, M):
    """y = resid + sum: the sum's bound and the add (u |y|)."""
    for resid in (np.random.default_rng(M).standard_normal((M, w.N)).astype(np.float32), None):
        y, _ = _run_resid(torch, w, hi, lo, resid)
        ref = R.epi_resid(Y, None, resid)
        tol = dY + R.EPS32 * (np.abs(Y) + (0.0 if resid is None else np.abs(resid)))
        _hold(fails, f"resid {resid is not None}", y, ref, tol)


@pytest.mark.parametrize("M", [64, 256])
@pytest.mark.parametrize("role,K", [(0, 704), (1, 704), (2, 704), (2, 4096)])
def test_realistic_values(gpu, tables, role, K, M):
    torch = gpu
    fails = []
    N = {0: 1344, 1: 2 * G.INTER, 2: G.N_RESID}[role]
    w = _real_weights(torch, N, K, 11 * M + role)
    hi, lo = _real_acts(torch, M, K, 5 * M + role)
    Y = R.gemm_sums(w.W, hi, lo)
    dY = 4 * R.EPS32 * np.sqrt(K) * R.gemm_abs(w.W, hi, lo)
    if role == 2:
        _check_resid_real(fails, torch, w, hi, lo, Y, dY, M)
    elif role == 1:
        for silu in (0, 1):
            got, _ = _run_swiglu(torch, w, hi, lo, silu)
            _check_swiglu(fails, f"silu {silu}", got, Y, dY, silu)
    else:
        p0, T = 5, M + 16
        for kv in ("f16", "f32"):
            out = _run_qkv(torch, tables, w, hi, lo, G.QKV, kv, p0, M, T)
            _check_qkv(fails, f"kv {kv}", tables, out, Y, dY, G.QKV, p0, M, T)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- 5. padding and bounds of the cache stores
def _bounds_cases(M):
    return [(0, M - 27, M + 8), (256, M, 256 + M + 8), (256, M - 20, 256 + M - 20), (256, M, 256 + M - 20)]


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("kv", ["f16", "f32"])
def test_qkv_cache_stores_stay_in_their_rows(gpu, tables, kv, case):
    torch = gpu
    M = 64
    p0, nv, T = _bounds_cases(M)[case]
    fails = []
    codes, scales, hi, lo = G.grid_inputs(1344, 128, M, 7 + case)
    w = Wmx(torch, codes, scales)
    Y = R.gemm_sums(w.W, hi, lo)
    out = _run_qkv(torch, tables, w, hi, lo, G.QKV, kv, p0, nv, T)
    _check_qkv(fails, f"p0 {p0} nv {nv} T {T}", tables, out, Y, None, G.QKV, p0, nv, T)
    written = ~_is_sentinel(out[1])[1].all(axis=(0, 2))  # rows of the layer with anything written
    assert np.array_equal(np.nonzero(written)[0], np.arange(p0, min(p0 + nv, T))), np.nonzero(written)[0]
    assert not np.isnan(out[0]).any()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- 6. argument checks (nothing is launched)
def test_entry_point_rejects_what_the_kernel_cannot_take(gpu):
    torch = gpu
    from simplellminference_amd import _lib, ops
    from simplellminference_amd._lib import SliError

    def rejected(fn, *a, **k):
        with pytest.raises(SliError) as e:
            fn(*a, **k)
        assert e.value.code == 1, e.value  # SLI_ERR_ARG

    def u8(*s):
        return torch.zeros(*s, dtype=torch.uint8, device="cuda")

    def f16(*s):
        return torch.zeros(*s, dtype=torch.float16, device="cuda")

    def f32(*s):
        return torch.zeros(*s, dtype=torch.float32, device="cuda")

    rejected(ops.prefill_gemm_resid, u8(64, 48), f16(32, 96), f16(32, 96), f32(32, 64), scales=u8(64, 3))   # K % 64
    rejected(ops.prefill_gemm_resid, u8(24, 32), f16(32, 64), f16(32, 64), f32(32, 24), scales=u8(24, 2))   # N % 16
    rejected(ops.prefill_gemm_resid, u8(64, 32), f16(48, 64), f16(48, 64), f32(48, 64), scales=u8(64, 2))   # M = 48
    with pytest.raises(ValueError):  # mis-shaped scales
        ops.prefill_gemm_resid(u8(64, 32), f16(32, 64), f16(32, 64), f32(32, 64), scales=u8(64, 4))
    with pytest.raises(ValueError):  # a row scale beside block scales
        ops.prefill_gemm_resid(u8(64, 32), f16(32, 64), f16(32, 64), f32(32, 64), scales=u8(64, 2), row_scale=f32(64))
    # sli_prefill_gemm itself keeps refusing the dtype
    y, state = f32(32, 64), torch.zeros(48, dtype=torch.int32, device="cuda")  # SLI_PF_TABLE_BYTES
    e = _lib.PgemmEpilogue(role=2, y=y.data_ptr(), resid=None, ld=64)
    with pytest.raises(SliError, match="MXFP4 have no GEMM prefill") as ei:
        _lib.call("sli_prefill_gemm", ops._p(u8(64, 32)), _lib.DT_MXFP4, None, ops._p(f16(32, 64)), ops._p(f16(32, 64)),
                  64, 64, 32, 0, 32, ctypes.byref(e), ops._p(state), None, ops._s())
    assert ei.value.code == 1
    tl = ops.prefill_gemm_resid(u8(64, 32), f16(32, 64), f16(32, 64), y, scales=u8(64, 2))  # and the smallest good call
    assert tl["BM"] == 32


# ---------------------------------------------------------------- 7. model level
MATS = ("T_WQ", "T_WK", "T_WV", "T_WO", "T_UP", "T_GATE", "T_DOWN")


def _ocfg(oracle, cfg):
    return oracle.Config(cfg.vocab_size, cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads,
                         cfg.head_dim, cfg.intermediate_size, cfg.num_hidden_layers, cfg.max_length,
                         cfg.rms_norm_eps, cfg.rope_theta)


def _mx_oracle(oracle, cfg, seed):
    """test_gpu_mxfp4.py's construction: an eager fp32 oracle whose embedding (the tied LM head) and seven matrices
    per layer were overwritten in place with the rule's dequantisation."""
    om = oracle.Model(_ocfg(oracle, cfg), seed=seed, wmode=oracle.W_F32, kv_f16=True)
    t = om.weight(oracle.T_EMB)
    t[...] = mx.quant_dequant(t)
    for l in range(cfg.num_hidden_layers):
        for name in MATS:
            w = om.weight(getattr(oracle, name), l)
            w[...] = mx.quant_dequant(w)
    return om


def _prompt(n, vocab, seed=3):
    return [int(t) for t in np.random.default_rng(seed + n).integers(0, vocab, n)]


def _min_top2_gap(logits):
    s = np.sort(logits, axis=-1)
    return float((s[..., -1] - s[..., -2]).min())


# Seeds chosen with the oracle alone, on the CPU: the minimum top-2 logit gap over the positions n - 1 .. of each run
# below must be >= 4e-3, four times the logit bar, so a difference inside the bar cannot flip a token. Scans:
#   tiny, n = (2, 33, 63), seeds 0-47: 21 is the first seed with every gap >= 4e-3 (5.3e-3, 1.2e-2, 1.3e-1; seeds 0-7
#     reach at most 3.4e-3 at n = 2, 62 greedy steps);
#   tiny-gqa, n = (2, 33, 63), seeds 0-7: 7 (5.9e-3, 4.5e-3, 7.2e-3), the only one;
#   tiny-gqa at max_length 320, n = (129, 300), seeds 0-7: 1 (1.2e-2, 9.6e-3);
#   tiny-gqa, intermediate_size 704, n = 150, seeds 0-7: 3 (1.1e-1);
#   tiny with hidden_size 320 (5 heads of 64), n = 150, seeds 0-7: 2 (3.2e-2), the largest;
#   tiny-h8 (the TP-2 run), n = 33, seeds 0-7: 5 (1.0e-1).
MODEL_RUNS = [
    ("tiny", {}, 21, 2), ("tiny", {}, 21, 33), ("tiny", {}, 21, 63),
    ("tiny-gqa", {}, 7, 2), ("tiny-gqa", {}, 7, 33), ("tiny-gqa", {}, 7, 63),
    ("tiny-gqa", dict(max_length=320), 1, 129), ("tiny-gqa", dict(max_length=320), 1, 300),
    ("tiny-gqa", dict(max_length=160, intermediate_size=704), 3, 150),  # down: 5.5 stages
    ("tiny", dict(max_length=160, hidden_size=320, kv_hidden_size=320, num_attention_heads=5,
                  num_key_value_heads=5), 2, 150),                      # qkv, gate/up, wo: 2.5 stages
]
MIN_GAP = 4e-3


def _check_run(gtok, glog, otok, olog, n):
    assert _min_top2_gap(olog[n - 1:]) >= MIN_GAP
    assert np.array_equal(gtok, otok), (gtok, otok)
    assert np.isnan(glog[:n - 1]).all()
    err = float(np.abs(glog[n - 1:] - olog[n - 1:]).max())
    print(f"max|dlogit| {err:.3e}")
    assert err <= 1e-3, err


@pytest.mark.parametrize("name,over,seed,n", MODEL_RUNS)
def test_model_gemm_prefill_matches_oracle(gpu, oracle, name, over, seed, n):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset(name, **over)
    steps = min(cfg.max_length, max(64, n + 12))
    prompt = _prompt(n, cfg.vocab_size)
    om = _mx_oracle(oracle, cfg, seed)
    otok, olog = om.predict(prompt, steps)
    ok, ov = (a.copy() for a in om.kv_cache())  # views of the oracle's memory: copied before close()
    om.close()
    gm = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=seed).init()
    gm.set_prefill("gemm")
    assert gm.prefill_path() == "mfma"
    gtok, glog = gm.predict_prefill(prompt, steps, want_logits=True)
    kv = [(gm.kv(layer, 0, n - 1), gm.kv(layer, 1, n - 1)) for layer in range(cfg.num_hidden_layers)] if n > 1 else []
    gm.close()
    _check_run(gtok, glog, otok, olog, n)
    for layer, (gk, gv) in enumerate(kv):  # rows 0 .. n-2 come from the prefill
        np.testing.assert_allclose(gk, ok[layer, :n - 1], rtol=0, atol=2e-3)
        np.testing.assert_allclose(gv, ov[layer, :n - 1], rtol=0, atol=2e-3)


def test_tp_group_gemm_prefill_matches_unsharded_oracle(gpu, oracle):
    """Two in-process ranks of tiny-h8: column shards of wo / down on 32-column blocks, the chunk's residual rows
    summed over the ranks after each."""
    from simplellminference_amd.model import TPGroup, preset
    cfg, seed, n, steps = preset("tiny-h8"), 5, 33, 64
    prompt = _prompt(n, cfg.vocab_size)
    om = _mx_oracle(oracle, cfg, seed)
    otok, olog = om.predict(prompt, steps)
    ok, ov = (a.copy() for a in om.kv_cache())  # views of the oracle's memory: copied before close()
    om.close()
    g = TPGroup(cfg, tp_size=2, w_dtype="mxfp4", kv_dtype="f16", seed=seed).init()
    assert g.prefill_path() == "decode"
    g.set_prefill("gemm")
    assert g.prefill_path() == "mfma"
    gtok, glog = g.predict_prefill(prompt, steps, want_logits=True)
    kv = [[np.concatenate([m.kv(layer, which, n - 1) for m in g.ranks], axis=-1) for which in (0, 1)]
          for layer in range(cfg.num_hidden_layers)]
    g.close()
    _check_run(gtok, glog, otok, olog, n)
    for layer, (gk, gv) in enumerate(kv):
        np.testing.assert_allclose(gk, ok[layer, :n - 1], rtol=0, atol=2e-3)
        np.testing.assert_allclose(gv, ov[layer, :n - 1], rtol=0, atol=2e-3)


# Oracle-only scan of this run (CPU), seeds 1-3: minimum top-2 gaps over positions 139 .. 143 of 7.2e-1, 1.1e-1, 7.4e-2.
SEED_7B = 1


@pytest.mark.timeout(400)
def test_llama7b_layer_gemm_prefill(gpu, oracle):
    """One Llama-2-7B-shaped layer (vocabulary cut to 512 so the CPU oracle stays in budget), a 140-token prompt: one
    256-row chunk with 117 padding rows, hd 128, 4096 x 11008 projections (32 and 86 stages), then 4 greedy steps."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b", num_hidden_layers=1, vocab_size=512, max_length=160)
    n, steps = 140, 144
    prompt = _prompt(n, cfg.vocab_size)
    om = _mx_oracle(oracle, cfg, SEED_7B)
    otok, olog = om.predict(prompt, steps)
    ok, ov = (a.copy() for a in om.kv_cache())  # views of the oracle's memory: copied before close()
    om.close()
    gm = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=SEED_7B).init()
    gm.set_prefill("gemm")
    assert gm.prefill_path() == "mfma"
    gtok, glog = gm.predict_prefill(prompt, steps, want_logits=True)
    gk, gv = gm.kv(0, 0, n - 1), gm.kv(0, 1, n - 1)
    gm.close()
    _check_run(gtok, glog, otok, olog, n)
    np.testing.assert_allclose(gk, ok[0, :n - 1], rtol=0, atol=2e-3)
    np.testing.assert_allclose(gv, ov[0, :n - 1], rtol=0, atol=2e-3)


# ---------------------------------------------------------------- 8. the knob
def test_prefill_mode_knob(gpu):
    from simplellminference_amd._lib import SliError
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    prompt = _prompt(33, cfg.vocab_size)
    m = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=7).init()
    assert m.prefill_path() == "decode"  # the default stays the decode step for MXFP4
    runs = []
    for mode, path in (("gemm", "mfma"), ("decode", "decode"), ("gemm", "mfma"), ("auto", "decode"), ("gemm", "mfma")):
        m.set_prefill(mode)
        assert m.prefill_path() == path, (mode, m.prefill_path())
        m.reset()
        runs.append(m.predict_prefill(prompt, 64))
    for r in runs[1:]:  # flipping the mode between prefills of one model: the same tokens each time
        assert np.array_equal(r, runs[0])
    with pytest.raises(KeyError):
        m.set_prefill("mfma")  # not a mode
    m.close()
    h = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=7).init()
    assert h.prefill_path() == "mfma"
    a = h.predict_prefill(prompt, 64)
    h.reset()
    h.set_prefill("decode")
    assert h.prefill_path() == "decode"
    b = h.predict_prefill(prompt, 64)
    h.reset()
    h.set_prefill("auto")
    assert h.prefill_path() == "mfma"
    assert np.array_equal(a, b) and np.array_equal(a, h.predict_prefill(prompt, 64))
    h.close()
    f = LlamaModel(config=cfg, w_dtype="f32", kv_dtype="f32", seed=7).init()
    with pytest.raises(SliError, match="cannot take the GEMM prefill") as ei:
        f.set_prefill("gemm")
    assert ei.value.code == 7  # SLI_ERR_STATE
    assert f.prefill_path() == "decode"
    f.close()
