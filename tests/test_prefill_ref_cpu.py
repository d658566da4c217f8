"""tests/prefill_ref.py (the float64 reference of the prefill kernels) against the C oracle, one small case per
stage, within the bars test_oracle.py holds the oracle's own operators to; and the grid-input generators against
the conditions they state. No GPU: the reference is known good before test_gpu_prefill_kernels.py uses it.
"""
import numpy as np
import pytest

from tests import prefill_ref as R


def _rng(seed):
    return np.random.default_rng(seed)


def test_norm_and_split_match_oracle_rmsnorm(oracle):
    r = _rng(1)
    x = r.standard_normal((3, 320)).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(320)).astype(np.float32)
    h = R.norm(x, w, 1e-5)
    for m in range(3):
        np.testing.assert_allclose(oracle.rmsnorm(x[m], w, 1e-5), h[m], rtol=1e-6, atol=1e-6)
    assert np.array_equal(R.norm(x, None, 1e-5), x.astype(np.float64))
    hi, lo = R.split(h.astype(np.float32))
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    np.testing.assert_allclose(R.joined(hi, lo), h.astype(np.float32), rtol=R.SPLIT_REL, atol=R.SPLIT_ABS)
    assert np.all(np.abs(lo.astype(np.float64)) <= 2.0 ** -11 * np.abs(hi.astype(np.float64)))


@pytest.mark.parametrize("p0,nv,T", [(0, 4, 64), (37, 3, 40)])
def test_gemm_qkv_matches_oracle_matmul_and_rope(oracle, p0, nv, T):
    """Y = W (hi + lo) against oracle.matmul on the unsplit fp32 row (the split loses 2^-22 of it), the epilogue
    against oracle.rope at p0 + m; rows past nv or T are not stored."""
    hq, hkv, hd, K, M = 4, 2, 64, 128, 4
    r = _rng(2 + p0)
    x = r.standard_normal((M, K)).astype(np.float32)
    W = (r.standard_normal(((hq + 2 * hkv) * hd, K)) / np.sqrt(K)).astype(np.float16)
    hi, lo = R.split(x)
    Y = R.gemm_sums(W, hi, lo)
    sin_t, cos_t = oracle.rope_cache(hd, T, 10000.0)
    q, k, v, stored = R.epi_qkv(Y, None, sin_t, cos_t, p0, nv, T, hq, hkv, hd)
    assert stored.tolist() == [m < nv and p0 + m < T for m in range(M)]
    nq, nk = hq * hd, hkv * hd
    for m in range(M):
        y = oracle.matmul(x[m], W.astype(np.float32))
        np.testing.assert_allclose(y, Y[m], rtol=0, atol=1e-5)
        oq, ok = oracle.rope(y[:nq].copy(), y[nq:nq + nk].copy(), min(p0 + m, T - 1), sin_t, cos_t, hd)
        np.testing.assert_allclose(oq, q[m], rtol=0, atol=1e-5)
        np.testing.assert_allclose(ok, k[m].ravel(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(y[nq + nk:], v[m].ravel(), rtol=0, atol=1e-5)
    # the error model of the RoPE: the oracle's fp32 rotation of exact inputs sits inside rope_tol
    a = Y.astype(np.float32)
    pos = np.minimum(p0 + np.arange(M), T - 1)
    want = R.rope_rows(a[:, :nq], pos, sin_t, cos_t, hd)
    tol = R.rope_tol(a[:, :nq], pos, sin_t, cos_t, hd)
    for m in range(M):
        oq, _ = oracle.rope(a[m, :nq].copy(), a[m, nq:nq + nk].copy(), int(pos[m]), sin_t, cos_t, hd)
        assert np.all(np.abs(oq - want[m]) <= tol[m])


def test_gemm_row_scales_swiglu_and_resid_match_oracle(oracle):
    inter, K, M = 24, 64, 3
    r = _rng(5)
    x = r.standard_normal((M, K)).astype(np.float32)
    Wf = (r.standard_normal((2 * inter, K)) / np.sqrt(K)).astype(np.float32)
    Wq = np.empty((2 * inter, K), np.int8)
    s = np.empty(2 * inter, np.float32)
    for i in range(2 * inter):
        Wq[i], s[i] = oracle.quant_row_i8(Wf[i])
    hi, lo = R.split(x)
    Y = R.gemm_sums(Wq, hi, lo)
    deq = Wq.astype(np.float32) * s[:, None]
    resid = r.standard_normal((M, 2 * inter)).astype(np.float32)
    for silu in (0, 1):
        a = R.epi_swiglu(Y, s, inter, silu)
        for m in range(M):
            y = oracle.matmul(x[m], deq)
            np.testing.assert_allclose(y, Y[m] * s, rtol=0, atol=1e-5)
            g, u = y[:inter].copy(), y[inter:].copy()
            want = oracle.swiglu(u, g) * (g if silu else 1.0)
            np.testing.assert_allclose(want, a[m], rtol=1e-5, atol=1e-6)
            # the error model of the activation: the oracle's fp32 sigmoid(g) * u of exact g, u sits inside act_tol
            # less its hi/lo split terms
            exact = R.act(g.astype(np.float64), u.astype(np.float64), 0)
            assert np.all(np.abs(oracle.swiglu(u, g) - exact) <= 4 * R.EPS32 * np.abs(exact) + 1e-45)
    out = R.epi_resid(Y, s, resid)
    for m in range(M):
        np.testing.assert_allclose(oracle.add(resid[m], oracle.matmul(x[m], deq)), out[m], rtol=0, atol=1e-5)
    assert np.array_equal(R.epi_resid(Y, None, None), Y)


@pytest.mark.parametrize("hq,hkv", [(2, 2), (4, 1)])
def test_attention_matches_oracle_mha_query_by_query(oracle, hq, hkv):
    hd, T, p0, M = 64, 24, 17, 9  # chunk rows 7, 8 lie past T
    r = _rng(hq)
    q = r.standard_normal((M, hq * hd)).astype(np.float32)
    K = r.standard_normal((hkv, T, hd)).astype(np.float16).astype(np.float32)
    V = r.standard_normal((hkv, T, hd)).astype(np.float16).astype(np.float32)
    out = R.attn(q, K, V, p0, hq, hkv, hd)
    kc = np.ascontiguousarray(K.transpose(1, 0, 2).reshape(1, T, hkv * hd))  # reference layout [L][T][KV]
    vc = np.ascontiguousarray(V.transpose(1, 0, 2).reshape(1, T, hkv * hd))
    for m in range(M):
        if p0 + m >= T:
            assert np.isnan(out[m]).all()
            continue
        want = oracle.mha(q[m], kc, vc, 0, p0 + m, T, hd, hq, hkv)
        np.testing.assert_allclose(want, out[m], rtol=0, atol=1e-5)


@pytest.mark.parametrize("int8", [False, True])
def test_grid_inputs_meet_their_conditions(int8):
    """The largest case of the GPU file (256 x 1344 x 1024) and the 4096-deep one: values on the grid, hi and lo
    independent, sum |W| (|hi| + |lo|) in grid units below 2^24, and (on a slice) fp32 sums exact in any order."""
    for (N, K, M) in [(1344, 1024, 256), (1168, 1024, 256), (1152, 1024, 256), (64, 4096, 32)]:
        W, scale, hi, lo = R.grid_inputs(N, K, M, int8, seed=N + K)
        if int8:
            assert W.dtype == np.int8 and np.abs(W.astype(int)).max() <= 8
            e = np.log2(scale.astype(np.float64))
            assert scale.dtype == np.float32 and np.array_equal(e, np.round(e)) and e.min() >= -7 and e.max() <= -5
        else:
            k = W.astype(np.float64) * R.GRID_W
            assert W.dtype == np.float16 and scale is None and np.array_equal(k, np.round(k)) and np.abs(k).max() <= 8
        for h in (hi, lo):
            k = h.astype(np.float64) * R.GRID_H
            assert h.dtype == np.float16 and np.array_equal(k, np.round(k)) and np.abs(k).max() <= 8
        # independent draws, not a split of one vector: lo is as large as hi, and uncorrelated with it
        assert np.mean(np.abs(lo.astype(np.float64)) > 2.0 ** -11 * np.abs(hi.astype(np.float64))) > 0.8
        assert abs(np.corrcoef(hi.astype(np.float64).ravel(), lo.astype(np.float64).ravel())[0, 1]) < 0.02
        assert np.abs(lo.astype(np.float64)).sum() > 0.9 * np.abs(hi.astype(np.float64)).sum()
        units = R.grid_units(W, hi, lo)
        assert units == np.round(units) and units < 2 ** 24, units
    W, scale, hi, lo = R.grid_inputs(48, 1024, 32, int8, seed=9)
    Y = R.gemm_sums(W, hi, lo)
    terms = (W.astype(np.float32)[None, :, :] * (hi.astype(np.float32) + lo.astype(np.float32))[:, None, :])
    perm = _rng(0).permutation(1024)
    for t in (terms, terms[:, :, perm], terms[:, :, ::-1]):
        acc = np.zeros(t.shape[:2], np.float32)
        for kk in range(t.shape[2]):  # a sequential fp32 sum in this order
            acc += t[:, :, kk]
        assert np.array_equal(acc.astype(np.float64), Y)
    resid = R.grid_resid(32, 48, 3)
    out = R.epi_resid(Y, scale, resid)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)  # representable: the fp32 epilogue is exact


def test_f16_rounding_interval():
    ref = np.array([1.0, 1.0 + 2.0 ** -11, 0.1, -3.3])
    got = ref.astype(np.float16)
    assert R.within_f16_rounding(got, ref, 0.0).all()
    up = np.nextafter(got, np.float16(np.inf))
    assert not R.within_f16_rounding(up, ref, 1e-9)[[0, 2, 3]].any()
    # a tie: an fp32 error of either sign decides the rounding, both neighbours are acceptable, nothing further
    assert R.within_f16_rounding(np.float16([1.0, 1.0 + 2.0 ** -10]), ref[1], 1e-7).all()
    assert not R.within_f16_rounding(np.float16(1.0 + 2.0 ** -9), ref[1], 1e-7)
