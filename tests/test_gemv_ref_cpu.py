"""tests/gemv_ref.py (the float64 reference of one batch-1 decode GEMV launch) against the C oracle's rmsnorm, matmul,
rope, swiglu and mha, at the bars test_bgemm_ref_cpu.py holds bgemm_ref to; the generators against the conditions they
state. No GPU: the reference is known good before test_gpu_decode_gemv.py uses it.
"""
import numpy as np
import pytest

from tests import bgemm_ref as B
from tests import gemv_ref as G
from tests import prefill_ref as P


def _rng(seed):
    return np.random.default_rng(seed)


def test_norm_before_the_products_matches_oracle_rmsnorm_matmul(oracle):
    K, N, eps = 320, 48, 1e-5
    r = _rng(1)
    x = r.standard_normal(K).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    for wt in G.WTS:
        W, rs, Wv = G.real_weights(N, K, wt, 2)
        assert np.array_equal(Wv, G.w64(W, wt))
        h, inv = G.staged_norm(x, w, eps)
        ho = oracle.rmsnorm(x, w, eps)
        np.testing.assert_allclose(ho, h, rtol=1e-6, atol=1e-6)
        assert (np.abs(ho - h) <= G.staged_norm_tol(h) + 1e-12).all()  # the oracle's fp32 chain is inside the bound
        Y, A = G.sums(Wv, h)
        a, _ = G.scaled(Y, np.zeros(N), rs)
        deq = Wv.astype(np.float32) * (1.0 if rs is None else rs[:, None])
        np.testing.assert_allclose(oracle.matmul(ho, deq), a, rtol=0, atol=1e-5)
        assert (A >= np.abs(Y)).all()


def test_x1_sum_order_and_kpart_view():
    r = _rng(3)
    x = r.standard_normal(64).astype(np.float32)
    parts = r.standard_normal((4, 64)).astype(np.float32)
    v = G.x1_sum(x, parts)
    assert np.array_equal(v, (((x + parts[0]) + parts[1]) + parts[2]) + parts[3])
    assert np.array_equal(G.x1_sum(x, None), x)
    np.testing.assert_allclose(v, x.astype(np.float64) + parts.astype(np.float64).sum(axis=0), rtol=0, atol=1e-6)
    Wv, h = r.standard_normal((6, 64)), r.standard_normal(64)
    for ks in (2, 4):
        Wk, kc = G.kpart_view(Wv, ks), 64 // ks
        tot = sum(Wk[k] @ h[k * kc:(k + 1) * kc] for k in range(ks))
        np.testing.assert_allclose(tot, Wv @ h, rtol=0, atol=1e-12)
        assert np.array_equal(Wk[1][2], Wv[2, kc:2 * kc])


@pytest.mark.parametrize("hq,hkv,hd", [(4, 2, 64), (2, 2, 128)])
def test_rope_and_swiglu_match_oracle(oracle, hq, hkv, hd):
    T = 40
    r = _rng(hd)
    a = r.standard_normal((hq + 2 * hkv) * hd)
    sin_t, cos_t = oracle.rope_cache(hd, T, 10000.0)
    nq, nk = hq * hd, hkv * hd
    for pos in (0, 17, T - 1):
        ps = np.array([pos])
        q = P.rope_rows(a[None, :nq], ps, sin_t, cos_t, hd)[0]
        k = P.rope_rows(a[None, nq:nq + nk], ps, sin_t, cos_t, hd)[0]
        oq, ok = oracle.rope(a[:nq].astype(np.float32), a[nq:nq + nk].astype(np.float32), pos, sin_t, cos_t, hd)
        np.testing.assert_allclose(oq, q, rtol=0, atol=1e-5)
        np.testing.assert_allclose(ok, k, rtol=0, atol=1e-5)
    g, u = a[:nq], a[nq:2 * nq] if hkv * 2 >= hq else a[:nq][::-1]
    np.testing.assert_allclose(oracle.swiglu(u.astype(np.float32), g.astype(np.float32)), P.act(g, u, 0), rtol=0, atol=1e-6)


@pytest.mark.parametrize("hd,ppwg,pos,max_splits", [(64, 4, 0, 3), (64, 4, 9, 3), (128, 8, 39, 5), (64, 4, 39, 8)])
def test_merge_is_mha_softmax_weighted_sum(oracle, hd, ppwg, pos, max_splits):
    """Per-split partials (o_s, m_s, l_s) of a real attention, merged by gemv_ref.merge over the live splits, are
    mha's own output: the softmax-weighted sum of the value rows."""
    T, heads = 40, 3
    r = _rng(pos + hd)
    q = r.standard_normal(heads * hd).astype(np.float32)
    kc = r.standard_normal((1, T, heads * hd)).astype(np.float32)
    vc = r.standard_normal((1, T, heads * hd)).astype(np.float32)
    want = oracle.mha(q, kc, vc, 0, pos, T, hd, heads, heads)
    ns = G.live_splits(pos, ppwg, max_splits)
    part = np.full((heads, max_splits, hd + 4), np.nan, np.float32)
    for h in range(heads):
        sl = slice(h * hd, (h + 1) * hd)
        s = kc[0, :pos + 1, sl].astype(np.float64) @ q[sl] / np.sqrt(hd)
        for sp in range(ns):
            lo, hi = sp * ppwg, (pos + 1 if sp == ns - 1 else (sp + 1) * ppwg)
            m = s[lo:hi].max()
            e = np.exp(s[lo:hi] - m)
            part[h, sp, :hd] = e @ vc[0, lo:hi, sl]
            part[h, sp, hd], part[h, sp, hd + 1] = m, e.sum()
    got, tol = G.merge(part, ns, hd)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    assert np.isfinite(got).all() and (tol > 0).all() and tol.max() < 1e-4
    # the kernel's own fp32 chain (expf, fma per split in split order, one division) stays inside the bound
    p32 = part[:, :ns]
    M = p32[:, :, hd].max(axis=1, keepdims=True)
    w = np.exp((p32[:, :, hd] - M).astype(np.float32)).astype(np.float32)
    o, L = np.zeros((heads, hd), np.float32), np.zeros(heads, np.float32)
    for sp in range(ns):
        o = (w[:, sp, None].astype(np.float64) * p32[:, sp, :hd] + o).astype(np.float32)
        L = (w[:, sp].astype(np.float64) * p32[:, sp, hd + 1] + L).astype(np.float32)
    assert (np.abs((o / L[:, None]).reshape(-1).astype(np.float64) - got) <= tol).all()


def test_exact_generators_state_their_conditions():
    for K in (64, 256, 2720, 2736, 4096, 11008):
        x = G.exact_x_norm(K, K)  # asserts inv == 0.25 itself
        assert float(B.inv_rms(x[None, :], 0.0)[0]) == 0.25
        assert set(np.unique(G.exact_norm_w(K, K))) <= {1.0, 2.0}
    for wt in G.WTS:
        W, rs, Wv, unit = G.exact_weights(24, 256, wt, 5)
        assert np.array_equal(Wv, G.w64(W, wt)) and np.array_equal(Wv / unit, np.round(Wv / unit))
        h = G.exact_x_norm(256, 5).astype(np.float64) * 0.25
        assert G.exact_units(Wv, h, unit * 0.25) < 2 ** 24
        with pytest.raises(AssertionError):
            G.exact_units(Wv, h + 1e-3, unit * 0.25)
    for ns in range(1, 17):
        part = G.exact_merge_parts(2, 16, 64, ns, ns)
        h, _ = G.merge(part, ns, 64)
        assert np.isnan(part[:, ns:]).all() and np.isnan(part[:, :, 66:]).all()
        want = part[:, :ns, :64].astype(np.float64).sum(axis=1).reshape(-1) / 2.0 ** max(ns - 1, 0)
        assert np.array_equal(h, want) and B.is_f32(h)
        assert np.array_equal(h / 2.0 ** -(ns - 1) if ns > 1 else h, np.round(h / 2.0 ** -(ns - 1) if ns > 1 else h))


def test_wave_items_partition_every_unit():
    for grid, units, cs, cw in ((2, 86, 1, 16), (230, 11008, 1, 16), (256, 6144, 1, 12), (3, 7, 4, 16), (1, 1100, 1, 16)):
        items = G.wave_items(dict(grid=grid, units=units, csplit=cs, cw=cw))
        assert sum(map(sum, items)) == units * cs and len(items) == grid and all(len(w) == cw for w in items)
    assert G.merge_positions(16) == [0, 3, 4, 31, 32, 63] and G.merge_positions(3) == [0, 3, 4, 11]
    assert [G.live_splits(p, 4, 8) for p in (0, 3, 4, 31, 32)] == [1, 1, 2, 8, 8]
