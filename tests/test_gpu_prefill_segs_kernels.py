"""The two prefill stages that read a group table (csrc/prefill.h PfSegs; sli_model_prefill_seqs), one launch at a
time through ops.prefill_gemm_qkv_segs / ops.prefill_attn_segs, held to float64 through tests/prefill_ref.py.

A packed chunk's rows are 16-row groups (seq, p0, nv) of several sequences. Per-row arithmetic is that of the one-
sequence kernels (one body, parameterised on the row map), so the per-row bounds of tests/test_gpu_prefill_kernels.py
apply unchanged: grid sums are exact, q and K within prefill_ref.rope_tol (exact at position 0), what lands in an
fp16 cache within prefill_ref.within_f16_rounding, an FP8 cache holds the code of a value inside the same interval
(the encoder is monotone too), V rows are exactly the rounded sums; attention rtol 1e-5, atol 2e-6 per query
(test_gpu_prefill_kernels.py::test_prefill_attention_per_query). What the table adds is checked on top: which
sequence's cache a row reaches, at which position, and that nothing else is written.
"""
import numpy as np
import pytest

from tests import kv8_ref as K8
from tests import mxfp4_prefill_ref as G
from tests import mxfp4_ref as mx
from tests import prefill_pack_ref as P
from tests import prefill_ref as R

pytestmark = pytest.mark.gpu

SENT16, SENT8, SENT32 = 0x7E5A, 0x7F, 0x7FC5A5A5  # NaN patterns no kernel result equals
TABLE = [(2, 0, 16), (0, 16, 5), (1, 0, 1), (0, 0, 16)]  # 3 sequences; the rest of the chunk is padding
B = 3


def _t(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def tables(gpu):
    from simplellminference_amd import ops
    out = {}
    for hd in (64, 128):
        s, c = ops.rope_cache(hd, 64, 10000.0)
        out[hd] = (s, c, s.cpu().numpy(), c.cpu().numpy())
    return out


def _cache(torch, shape, kv):
    if kv == "f16":
        return torch.full(shape, SENT16, dtype=torch.int16, device="cuda").view(torch.float16)
    return torch.full(shape, SENT8, dtype=torch.uint8, device="cuda")


def _weights(torch, w, N, K, M, seed):
    """Grid operands (exact sums in any order): (device weight, ops keyword arguments, float64 weights with the row
    scale folded in, hi, lo)."""
    if w == "mxfp4":
        codes, scales, hi, lo = G.grid_inputs(N, K, M, seed)
        return _t(torch, mx.pack(codes)), {"scales": _t(torch, scales)}, G.weights64(codes, scales), hi, lo
    W, scale, hi, lo = R.grid_inputs(N, K, M, w == "i8", seed)
    W64 = W.astype(np.float64) * (1.0 if scale is None else scale.astype(np.float64)[:, None])
    return _t(torch, W), ({"row_scale": _t(torch, scale)} if scale is not None else {}), W64, hi, lo


def _run(torch, tables, Wd, kw, hi, lo, groups, hq, hkv, hd, T, kv):
    from simplellminference_amd import ops
    M = hi.shape[0]
    sin_d, cos_d, _, _ = tables[hd]
    q = torch.full((M, hq * hd), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    kc, vc = _cache(torch, (B, hkv, T, hd), kv), _cache(torch, (B, hkv, T, hd), kv)
    ops.prefill_gemm_qkv_segs(Wd, _t(torch, hi), _t(torch, lo), q, kc, vc, sin_d[:T], cos_d[:T], hq, hkv, hd, groups,
                              kv_dtype="f8" if kv == "f8" else None, **kw)
    return q.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy()


def _check(tables, out, Y, dY, groups, hq, hkv, hd, T):
    """q and the caches against the restatement of the float64 sums Y known to +- dY (None: exact)."""
    q, kc, vc = out
    _, _, sin_t, cos_t = tables[hd]
    sin_t, cos_t = sin_t[:T], cos_t[:T]
    M, nq, nk = Y.shape[0], hq * hd, hkv * hd
    q_ref, stores = P.epi_qkv_segs(Y, None, sin_t, cos_t, groups, T, hq, hkv, hd)
    pos = np.concatenate([np.minimum((groups[g][1] if g < len(groups) else 0) + np.arange(16), T - 1)
                          for g in range(M // 16)])
    tol_q = R.rope_tol(Y[:, :nq], pos, sin_t, cos_t, hd, None if dY is None else dY[:, :nq])
    tol_k = R.rope_tol(Y[:, nq:nq + nk], pos, sin_t, cos_t, hd, None if dY is None else dY[:, nq:nq + nk])
    tol_v = np.zeros((M, nk)) if dY is None else dY[:, nq + nk:]
    if dY is None:  # sin 0 = 0, cos 0 = 1: the rotation at position 0 is exact
        tol_q[pos == 0] = 0.0
        tol_k[pos == 0] = 0.0
    err = np.abs(q.astype(np.float64) - q_ref)
    assert np.all(err <= tol_q), f"q: max excess {np.nanmax(err - tol_q):.3e}"  # every chunk row, padding included
    # the row of the chunk each store came from, in the order epi_qkv_segs lists them
    src = [16 * g + r for g in range(len(groups)) for r in range(groups[g][2]) if groups[g][1] + r < T]
    assert len(src) == len(stores) > 0
    written = np.zeros((B, T), bool)
    for m, (seq, p, k_ref, v_ref) in zip(src, stores):
        assert not written[seq, p]
        written[seq, p] = True
        for name, cache, ref, tol in (("k", kc, k_ref, tol_k[m].reshape(hkv, hd)), ("v", vc, v_ref, tol_v[m].reshape(hkv, hd))):
            got = cache[seq, :, p, :]
            if cache.dtype == np.float16:
                ok = R.within_f16_rounding(got, ref, tol)
            else:  # the codec is monotone as well: the code of some value in ref +- tol
                val = K8.decode(got).astype(np.float64)
                ok = (K8.decode(K8.encode(ref - tol)) <= val) & (val <= K8.decode(K8.encode(ref + tol)))
            assert ok.all(), f"{name} of sequence {seq} at position {p} (chunk row {m}): {int((~ok).sum())} outside"
    # every other byte of both caches is the sentinel: sequences no group names, rows >= nv, positions >= T
    for name, cache in (("k", kc), ("v", vc)):
        sent = (cache.view(np.uint16) == SENT16) if cache.dtype == np.float16 else (cache == SENT8)
        rows_written = ~sent.all(axis=(1, 3))  # [B][T]
        assert np.array_equal(rows_written, written), (name, np.argwhere(rows_written != written).tolist())


QKV_CASES = [(w, kv, hd, hkv, M, T) for w in ("f16", "i8") for kv in ("f16", "f8") for hd, hkv in ((64, 1), (128, 2))
             for M, T in ((64, 20), (128, 48))] + [("mxfp4", "f16", 64, 2, 64, 20), ("f16", "f8", 64, 2, 128, 20)]


@pytest.mark.parametrize("w,kv,hd,hkv,M,T", QKV_CASES)
def test_qkv_table_epilogue_grid(gpu, tables, w, kv, hd, hkv, M, T):
    """Exact grid sums through the table epilogue: group (0, 16, 5) at T = 20 straddles T (position 20 is dropped),
    sequence 1 gets one row, sequence 0 two groups out of order, and the chunk's other groups are padding."""
    torch = gpu
    hq = 2 * hkv
    N = (hq + 2 * hkv) * hd
    Wd, kw, W64, hi, lo = _weights(torch, w, N, 128, M, 17 * M + hd)
    Y = R.joined(hi, lo) @ W64.T
    out = _run(torch, tables, Wd, kw, hi, lo, TABLE, hq, hkv, hd, T, kv)
    _check(tables, out, Y, None, TABLE, hq, hkv, hd, T)


@pytest.mark.parametrize("w", ["f16", "i8"])
def test_qkv_table_epilogue_realistic(gpu, oracle, tables, w):
    """N(0, 1) activations, N(0, 1/K) weights, K = 704: the sum known to 4 eps32 sqrt(K) (|W| @ (|hi| + |lo|)), the
    bar of test_gpu_prefill_kernels.py::test_realistic_values, then epi_qkv per group at that group's p0."""
    torch = gpu
    from tests.test_gpu_prefill_kernels import _real_acts, _real_weights
    hq, hkv, hd, M, T, Kd = 4, 2, 64, 64, 48, 704
    N = (hq + 2 * hkv) * hd
    W, scale = _real_weights(oracle, N, Kd, w == "i8", 5)
    hi, lo = _real_acts(torch, M, Kd, 6)
    sc = 1.0 if scale is None else scale.astype(np.float64)
    Y = R.gemm_sums(W, hi, lo) * sc
    dY = 4 * R.EPS32 * np.sqrt(Kd) * R.gemm_abs(W, hi, lo) * sc + (R.U32 * np.abs(Y) if scale is not None else 0.0)
    kw = {"row_scale": _t(torch, scale)} if scale is not None else {}
    out = _run(torch, tables, _t(torch, W), kw, hi, lo, TABLE, hq, hkv, hd, T, "f16")
    _check(tables, out, Y, dY, TABLE, hq, hkv, hd, T)


# (groups, T): p0 0, 16 and 240 against a full cache; a group whose last position clamps to T - 1; padding groups in
# the middle of the table and at its end
ATTN_TABLES = [
    ([(1, 0, 16), (0, 16, 16), (2, 240, 16), (1, 16, 7)], 256),
    ([(0, 0, 16), (2, 0, 0), (1, 32, 9), (0, 0, 0)], 40),       # (1, 32, 9): positions 32 .. 47 of 40
    ([(2, 240, 16), (0, 0, 0), (0, 0, 0), (2, 224, 16), (1, 0, 3), (0, 128, 16), (0, 0, 0), (0, 0, 0)], 256),
]


@pytest.mark.parametrize("case", range(len(ATTN_TABLES)))
@pytest.mark.parametrize("kv,hd,hq,hkv", [("f16", 64, 2, 2), ("f16", 128, 4, 2), ("f16", 64, 8, 2), ("f8", 64, 4, 2),
                                          ("f8", 128, 2, 2), ("f8", 128, 8, 2)])
def test_attention_table_per_query(gpu, kv, hd, hq, hkv, case):
    """Group g's rows equal float64 attention over ITS sequence's cache at ITS p0; the sequences' caches differ by
    large offsets, so a wrong base or position shows at once. Rows of padding groups are not compared (and stay
    as the output buffer was), rows at positions >= T neither."""
    torch = gpu
    from simplellminference_amd import ops
    groups, T = ATTN_TABLES[case]
    M = 16 * len(groups)
    r = np.random.default_rng(100 * case + hd + hq)
    q = r.standard_normal((M, hq * hd)).astype(np.float32)
    Kc = r.standard_normal((B, hkv, T, hd)).astype(np.float32) + np.array([0.0, 3.0, -3.0])[:, None, None, None].astype(np.float32)
    Vc = r.standard_normal((B, hkv, T, hd)).astype(np.float32) + np.array([0.0, 40.0, -40.0])[:, None, None, None].astype(np.float32)
    if kv == "f16":
        Kc, Vc = Kc.astype(np.float16), Vc.astype(np.float16)
        Kv, Vv, kw = Kc, Vc, {}
    else:
        Kc, Vc = K8.encode(Kc), K8.encode(Vc)
        Kv, Vv, kw = K8.decode(Kc), K8.decode(Vc), {"kv_dtype": "f8"}
    ohi, olo = ops.prefill_attn_segs(_t(torch, q), _t(torch, Kc), _t(torch, Vc), groups, hq, hkv, hd, **kw)
    ohi, olo = ohi.cpu().numpy(), olo.cpu().numpy()
    got = R.joined(ohi, olo)
    compared = 0
    for g, (seq, p0, nv) in enumerate(groups):
        rows = slice(16 * g, 16 * g + 16)
        if nv == 0:
            assert not ohi[rows].any() and not olo[rows].any()  # the group left before writing anything
            continue
        ref = R.attn(q[rows], Kv[seq], Vv[seq], p0, hq, hkv, hd)
        n = min(16, T - p0)
        err = np.abs(got[rows][:n] - ref[:n])
        lim = 2e-6 + 1e-5 * np.abs(ref[:n])
        assert np.all(err <= lim), f"group {g} {seq, p0, nv}: max err {err.max():.3e}, worst err / lim {(err / lim).max():.2f}"
        compared += n
    assert compared >= 24


def test_entry_points_reject_bad_tables(gpu):
    """SLI_ERR_ARG, nothing launched; the good call in front shows each refusal is about the argument it names."""
    torch = gpu
    from simplellminference_amd import ops
    from simplellminference_amd._lib import SliError
    hq, hkv, hd, T, M = 2, 1, 64, 48, 32
    s, c = ops.rope_cache(hd, T, 10000.0)
    z = lambda dt, *sh: torch.zeros(*sh, dtype=dt, device="cuda")
    f16, f32 = torch.float16, torch.float32

    def qkv(groups=((0, 0, 16),), M_=M, cache=f16):
        return ops.prefill_gemm_qkv_segs(z(f16, 4 * hd, 64), z(f16, M_, 64), z(f16, M_, 64), z(f32, M_, hq * hd),
                                         z(cache, B, hkv, T, hd), z(cache, B, hkv, T, hd), s, c, hq, hkv, hd, groups)

    def attn(groups=((0, 0, 16),), M_=M, cache=f16):
        return ops.prefill_attn_segs(z(f32, M_, hq * hd), z(cache, B, hkv, T, hd), z(cache, B, hkv, T, hd), groups, hq,
                                     hkv, hd)

    for fn in (qkv, attn):
        fn()
        for bad in (dict(groups=[(0, 8, 16)]), dict(groups=[(0, 0, 16), (B, 0, 16)]), dict(groups=[(0, 0, 17)]),
                    dict(groups=[(-1, 0, 1)]), dict(groups=[(0, 48, 1)]), dict(cache=f32), dict(M_=48), dict(M_=16)):
            with pytest.raises(SliError) as e:
                fn(**bad)
            assert e.value.code == 1, (fn.__name__, bad, e.value)
    torch.cuda.synchronize()
