"""tests/bgemm_ref.py (the float64 reference of one batched decode projection launch) against the C oracle's
rmsnorm, matmul, rope, swiglu and add, within the bars test_oracle.py holds those operators to, and against
refmath's statements of the same operators; the generators and the recovery of the fp32 RMS factor against the
conditions they state. No GPU: the reference is known good before test_gpu_batch_kernels.py uses it.
"""
import numpy as np
import pytest

from tests import bgemm_ref as R
from tests import kv8_ref as F8
from tests import prefill_ref as P
from tests import refmath


def _rng(seed):
    return np.random.default_rng(seed)


def _launch(W, scale, x, norm_w, eps):
    Y, A = R.sums(W, x, norm_w)
    inv = R.inv_rms(x, eps) if norm_w is not None else None
    return Y, A, inv, R.scaled(Y, inv, scale)


def test_norm_factor_commutes_and_matches_oracle_rmsnorm_matmul(oracle):
    """sum_k W (x w) * inv == W @ rmsnorm(x, w): the launch applies the per-sequence factor to the finished sum."""
    B, K, N, eps = 3, 320, 48, 1e-5
    r = _rng(1)
    x = r.standard_normal((B, K)).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    W = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)
    Y, A, inv, a = _launch(W, None, x, w, eps)
    assert (A >= np.abs(Y)).all()
    for b in range(B):
        h = oracle.rmsnorm(x[b], w, eps)
        np.testing.assert_allclose(h, refmath.rmsnorm(x[b], w, eps), rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(h, R.staged(x, w)[b].astype(np.float64) * inv[b], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(oracle.matmul(h, W.astype(np.float32)), a[b], rtol=0, atol=1e-5)
        np.testing.assert_allclose(W.astype(np.float64) @ refmath.rmsnorm(x[b], w, eps), a[b], rtol=0, atol=1e-6)
    # no norm: the operand is x itself and there is no factor
    Y0, _, inv0, a0 = _launch(W, None, x, None, eps)
    assert inv0 is None and np.array_equal(Y0, a0)
    np.testing.assert_allclose(oracle.matmul(x[0], W.astype(np.float32)), a0[0], rtol=0, atol=1e-5)


@pytest.mark.parametrize("hq,hkv,hd", [(4, 2, 64), (2, 1, 128)])
def test_qkv_epilogue_matches_oracle_rope_per_sequence(oracle, hq, hkv, hd):
    B, K, T, eps = 3, 64, 40, 1e-5
    r = _rng(hd)
    x = r.standard_normal((B, K)).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    N = (hq + 2 * hkv) * hd
    Wf = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    Wq, s = np.empty((N, K), np.int8), np.empty(N, np.float32)
    for i in range(N):
        Wq[i], s[i] = oracle.quant_row_i8(Wf[i])
    pos = np.array([0, T - 1, 17])
    sin_t, cos_t = oracle.rope_cache(hd, T, 10000.0)
    _, _, _, a = _launch(Wq, s, x, w, eps)
    q, k, v = R.epi_qkv(a, pos, sin_t, cos_t, hq, hkv, hd)
    nq, nk = hq * hd, hkv * hd
    deq = Wq.astype(np.float32) * s[:, None]
    for b in range(B):
        y = oracle.matmul(oracle.rmsnorm(x[b], w, eps), deq)
        oq, ok = oracle.rope(y[:nq].copy(), y[nq:nq + nk].copy(), int(pos[b]), sin_t, cos_t, hd)
        np.testing.assert_allclose(oq, q[b], rtol=0, atol=1e-5)
        np.testing.assert_allclose(ok, k[b].ravel(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(y[nq + nk:], v[b].ravel(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(refmath.rope(a[b, :nq], int(pos[b]), sin_t, cos_t, hd), q[b], rtol=0, atol=1e-12)
    assert np.array_equal(q[0], a[0, :nq])  # position 0: the rotation is the identity


def test_swiglu_store_and_keys_match_oracle(oracle):
    B, K, inter, eps = 3, 96, 24, 1e-5
    r = _rng(5)
    x = r.standard_normal((B, K)).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    W = (r.standard_normal((2 * inter, K)) / np.sqrt(K)).astype(np.float16)
    _, _, _, a = _launch(W, None, x, w, eps)
    for silu in (0, 1):
        act = R.epi_swiglu(a, inter, silu)
        for b in range(B):
            y = oracle.matmul(oracle.rmsnorm(x[b], w, eps), W.astype(np.float32))
            g, u = y[:inter].copy(), y[inter:].copy()
            np.testing.assert_allclose(oracle.swiglu(u, g) * (g if silu else 1.0), act[b], rtol=1e-5, atol=1e-6)
            if not silu:
                np.testing.assert_allclose(refmath.swiglu(a[b, inter:], a[b, :inter]), act[b], rtol=0, atol=1e-12)
            # the error model: the oracle's fp32 sigmoid(g) * u of exact g, u sits inside swiglu_tol
            exact = P.act(g.astype(np.float64), u.astype(np.float64), 0)
            assert np.all(np.abs(oracle.swiglu(u, g) - exact) <= R.swiglu_tol(g.astype(np.float64), u.astype(np.float64), 0))
    Y0, _, _, a0 = _launch(W, None, x, None, eps)
    resid = r.standard_normal((B, 2 * inter)).astype(np.float32)
    out = R.epi_store(a0, resid, 0.5)
    for b in range(B):
        want = oracle.add(resid[b], oracle.matmul(x[b], W.astype(np.float32), 0.5))
        np.testing.assert_allclose(want, out[b], rtol=0, atol=1e-5)
    assert np.array_equal(R.epi_store(a0, None, 1.0), Y0)
    # keys: larger value, larger key; equal values (+-0 too), lower index wins; the parts decode
    row = np.array([1.0, -0.0, 3.5, 0.0, 3.5, -2.0, -np.inf], np.float32)
    keys = R.argmax_key(row, np.arange(7) + 1000)
    assert int(np.argmax(keys)) == 2 and int(np.argmax(keys)) == oracle.argmax(row)
    assert keys[1] > keys[3] and (keys[1] >> np.uint64(32)) == (keys[3] >> np.uint64(32))
    order = np.argsort(keys, kind="stable")
    assert row[order].tolist() == sorted(row.tolist())
    o, i = R.key_parts(R.best_key(row, 1000))
    assert int(i) == 1002 and int(o) == int(R.ordered(np.float32(3.5)))
    assert R.best_key(np.array([-0.0, 0.0], np.float32), 0) == int(R.argmax_key(np.float32(0.0), 0))


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("family", ["int", "lo"])
def test_exact_inputs_meet_their_conditions(int8, family):
    """The deepest and the widest cases of the GPU file: values on the grid, the staged operand exact, sum of absolute
    terms below 2^24 grid units, (on a slice) fp32 sums exact in any order, and for family "lo" a lo column whose loss
    changes most outputs."""
    for (N, K, B, norm) in [(512, 4096, 8, True), (70, 7168, 8, False), (80, 2560, 3, True), (560, 64, 8, True)]:
        W, scale, x, nw = R.exact_inputs(N, K, B, int8, family, norm, seed=N + K)
        assert (W.dtype == np.int8) == int8 and (scale is None) == (not int8)
        assert np.array_equal(W.astype(np.float64), np.round(W.astype(np.float64)))
        assert (nw is None) == (not norm)
        if norm:
            assert set(np.unique(nw)) <= {1.0, 2.0}
        if int8:
            assert np.array_equal(scale, 2.0 ** ((np.arange(N) % 5) - 2.0))
        assert R.exact_units(W, x, nw, family) < 2 ** 24
        if family == "lo":
            assert R.lo_matters(W, x, nw) > 0.9
            _, lo = P.split(R.staged(x, nw))
            assert np.mean(lo != 0) > 0.3
    W, scale, x, nw = R.exact_inputs(48, 1024, 8, int8, family, True, seed=9)
    Y, _ = R.sums(W, x, nw)
    assert R.is_f32(Y)
    terms = W.astype(np.float32)[None, :, :] * R.staged(x, nw)[:, None, :]
    perm = _rng(0).permutation(1024)
    for t in (terms, terms[:, :, perm], terms[:, :, ::-1]):
        acc = np.zeros(t.shape[:2], np.float32)
        for kk in range(t.shape[2]):  # a sequential fp32 sum in this order
            acc += t[:, :, kk]
        assert np.array_equal(acc.astype(np.float64), Y)
    # store: with grid residuals and a power-of-two scale the whole fp32 epilogue is exact
    W, scale, x, _ = R.exact_inputs(70, 1024, 8, int8, family, False, seed=3)
    Y, _ = R.sums(W, x, None)
    assert R.is_f32(R.epi_store(R.scaled(Y, None, scale), R.exact_resid(8, 70, 1), 0.5))


def test_recover_inv_finds_exactly_the_factor_used():
    """An fp32 factor 3 ulp off the float64 one is found from the outputs it produced; a row computed with another
    sequence's factor, or a factor outside 4 ulp, is not explained by any candidate."""
    W, scale, x, nw = R.exact_inputs(64, 544, 3, True, "int", True, seed=4)
    Y, _ = R.sums(W, x, nw)
    inv = R.inv_rms(x, 1e-5)
    assert len(R.inv_candidates(inv[0])) == 9
    used = R.inv_candidates(inv[1])[1]  # 3 ulp below
    got = R.apply_inv(Y[1], used, scale)
    assert R.recover_inv(got, Y[1], inv[1], scale) == used
    wrong = got.copy()
    wrong[5] = R.apply_inv(Y[1], np.float32(inv[2]), scale)[5]
    assert wrong[5] != got[5] and R.recover_inv(wrong, Y[1], inv[1], scale) is None
    far = np.float32(inv[1]) * np.float32(1 + 2.0 ** -20)
    assert R.recover_inv(R.apply_inv(Y[1], far, scale), Y[1], inv[1], scale) is None


def test_f8_acceptance_interval_and_flip_share():
    """f8_check takes the code of the reference, the neighbour only where ref +- tol straddles a boundary, nothing
    further, and the zero of the other sign only where the interval reaches it. On the GPU file's q/k/v inputs the
    share of cache elements whose interval straddles a boundary stays under kv8_ref.FLIP_CAP."""
    mid = F8.MIDS[0x40]
    ref = np.array([1.0, mid - 1e-9, mid + 1e-9, -(mid - 1e-9), 3e-12, 1.3])
    want = F8.encode(ref)
    ok, flip = R.f8_check(want, ref, 1e-7)
    assert ok.all() and not flip.any()
    nb = want.copy()
    nb[1] += 1
    nb[2] -= 1
    nb[3] += 1
    ok, flip = R.f8_check(nb, ref, 1e-7)
    assert ok.all() and flip[[1, 2, 3]].all()
    ok, _ = R.f8_check(nb, ref, 1e-10)
    assert not ok[[1, 2, 3]].any()
    ok, _ = R.f8_check(want + np.uint8(1), ref, 1e-7)
    assert not ok[[0, 5]].any()
    assert R.f8_check(np.uint8([0x80]), np.array([3e-12]), 1e-11)[0][0]       # -0 within reach
    assert not R.f8_check(np.uint8([0x80]), np.array([3e-12]), 1e-13)[0][0]  # -0 out of reach
    hq, hkv, hd, K, B, T = 4, 2, 64, 544, 8, 40
    sin_t, cos_t = refmath.rope_tables(hd, T, 10000.0)
    pos = (np.arange(B) * 5) % T
    for int8 in (False, True):
        W, scale, x, nw = R.exact_inputs((hq + 2 * hkv) * hd, K, B, int8, "lo", True, seed=K)
        Y, _ = R.sums(W, x, nw)
        a = R.scaled(Y, R.inv_rms(x, 1e-5), scale)
        _, k, v = R.epi_qkv(a, pos, sin_t, cos_t, hq, hkv, hd)
        for ref in (k, v):
            tol = 8 * R.EPS32 * np.abs(ref)
            _, lo, hi = R.f8_accept(ref, tol)
            assert np.mean(lo != hi) < F8.FLIP_CAP
