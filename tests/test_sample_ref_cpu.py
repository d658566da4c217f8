"""tests/sample_ref.py against the rule's text in include/sli.h: the hash, the uniforms, the candidate sets and the
distribution the rule draws from. No device."""
import numpy as np

from tests import sample_ref as R
from tests.test_oracle import _rng_u32  # the pure-Python sli_rng_u32 that test_oracle.py holds to the C generator


def test_hash_equals_the_header_generator():
    rng = np.random.default_rng(1)
    for seed, stream in ((0, 0), (7, (12 << 16) | 3), (0xFFFFFFFF, 0xFFFFFFFF), (12345, 12 << 16)):
        idx = np.concatenate([np.arange(8, dtype=np.uint64), rng.integers(0, 2 ** 63, 24, dtype=np.uint64) * np.uint64(2),
                              np.array([2 ** 32 - 1, 2 ** 32, (5 << 32) | 17, 2 ** 64 - 1], np.uint64)])
        got = R.rng_u32(seed, stream, idx)
        want = [_rng_u32(seed, stream, int(i)) for i in idx]
        assert [int(g) for g in got] == want


def test_uniforms_are_exact_fp32_inside_the_open_interval():
    for seed, seq, pos in ((0, 0, 0), (7, 3, 35), (2 ** 32 - 1, 65535, 2 ** 31 - 1)):
        u = R.uniforms(seed, seq, pos, 100000)
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
        assert u.min() > 0.0 and u.max() < 1.0
        assert u.min() >= 2.0 ** -24 and u.max() <= 1.0 - 2.0 ** -24
    # the extremes of h: never 0, never 1
    for h, want in ((0, 2.0 ** -24), (0xFFFFFFFF, 1.0 - 2.0 ** -24)):
        assert (2.0 * (h >> 9) + 1.0) * 2.0 ** -24 == want
    # the stream separates sequences, the counter positions
    a = R.uniforms(5, 0, 9, 64)
    assert not np.array_equal(a, R.uniforms(5, 1, 9, 64)) and not np.array_equal(a, R.uniforms(5, 0, 10, 64))
    assert not np.array_equal(a, R.uniforms(6, 0, 9, 64)) and np.array_equal(a, R.uniforms(5, 0, 9, 64))


def test_lower_set_inside_upper_set():
    rng = np.random.default_rng(2)
    for V, T, k, p in ((1000, 1.0, 0, 0.9), (1000, 0.3, 50, 0.5), (4096, 1.3, 0, 0.3), (257, 0.7, 10, 0.999)):
        l = rng.normal(0, 2.5, V).astype(np.float32)
        a = R.Acceptor(l, T, k, p)
        assert a.s_lo.any() and not (a.s_lo & ~a.s_hi).any() and not (a.s_hi & ~a.ck).any()
        assert a.s_hi[int(np.argmax(l))] and a.s_lo[int(np.argmax(l))]


def test_ties_at_the_k_boundary_are_kept():
    l = np.array([3, 1, 2, 2, 2, 0, -1], np.float32)
    assert R.top_k_set(l, 1).tolist() == [True, False, False, False, False, False, False]
    for k in (2, 3, 4):
        assert R.top_k_set(l, k).tolist() == [True, False, True, True, True, False, False]
    assert R.top_k_set(l, 5).tolist() == [True, True, True, True, True, False, False]
    assert R.top_k_set(l, 0).all() and R.top_k_set(l, 7).all() and R.top_k_set(l, 12).all()
    # -0 and +0 are one value
    z = np.array([1, -0.0, 0.0, -0.0, -5], np.float32)
    assert R.top_k_set(z, 2).tolist() == [True, True, True, True, False]
    # NaN and -inf are never candidates, and a NaN counts as -inf
    n = np.array([np.nan, 2, -np.inf, 1, np.nan], np.float32)
    assert R.top_k_set(n, 0).tolist() == [False, True, False, True, False]
    assert R.top_k_set(n, 1).tolist() == [False, True, False, False, False]
    assert R.top_k_set(n, 3).tolist() == [False, True, False, True, False]


def test_nucleus_keeps_ties_and_takes_the_smallest_prefix():
    l = np.log(np.array([0.4, 0.2, 0.2, 0.1, 0.1])).astype(np.float32)
    ck = np.ones(5, bool)
    assert R.nucleus(l, ck, 1.0, 0.3).tolist() == [True, False, False, False, False]
    assert R.nucleus(l, ck, 1.0, 0.5).tolist() == [True, True, True, False, False]   # the tie at 0.2 enters whole
    assert R.nucleus(l, ck, 1.0, 0.85).tolist() == [True] * 5
    assert R.nucleus(l, ck, 1.0, 1.0).tolist() == [True] * 5
    assert R.nucleus(l, ck, 1.0, 1e-6).tolist() == [True, False, False, False, False]


def test_degenerate_rows_follow_argmax():
    nan, inf = np.nan, np.inf
    assert R.draw(np.array([nan, nan, nan], np.float32), 1.0, 0, 1.0, 1, 0, 0) == 0
    assert R.draw(np.array([-inf, -inf], np.float32), 1.0, 0, 1.0, 1, 0, 0) == 0
    assert R.draw(np.array([-inf, nan, -inf], np.float32), 1.0, 0, 1.0, 1, 0, 0) == 0
    assert R.draw(np.array([1, inf, 5, inf], np.float32), 1.0, 0, 1.0, 1, 0, 0) == 1
    assert R.draw(np.array([nan, inf, 5], np.float32), 1.0, 0, 1.0, 1, 0, 0) == 0  # a NaN at index 0 is never displaced
    assert not R.degenerate(np.array([nan, 1, -inf], np.float32))


def test_fp32_evaluation_is_accepted_and_a_missing_stage_is_rejected():
    """The acceptance test passes an fp32 evaluation of the rule every time and catches an implementation that skips
    top-p or top-k (the issue's own experiment, at V = 4000 to stay quick)."""
    rng = np.random.default_rng(3)
    V = 4000
    l = rng.normal(0, 2.5, V).astype(np.float32)
    l[100:104] = l[100]
    for T, k, p in ((1.0, 0, 0.9), (0.7, 50, 0.5), (1.3, 40, 1.0)):
        a = R.Acceptor(l, T, k, p)
        bad_p = bad_k = 0
        for s in range(100):
            assert a.check(R.draw_fp32(l, T, k, p, 11, s, 5), 11, s, 5)[0]
            assert a.check(R.draw(l, T, k, p, 11, s, 5), 11, s, 5)[0]
            bad_p += not a.check(R.draw(l, T, k, 1.0, 11, s, 5), 11, s, 5)[0]
            bad_k += not a.check(R.draw(l, T, 0, p, 11, s, 5), 11, s, 5)[0]
        assert p == 1.0 or bad_p >= 3, (T, k, p, bad_p)
        assert k == 0 or bad_k >= 3, (T, k, p, bad_k)


def test_rule_draws_from_the_softmax():
    """20 000 reference draws at V = 50, T = 0.8 against softmax(l / T) by chi-square, bins of expected count below 5
    pooled. Seed 7 is fixed; the bound is the 1 - 1e-6 quantile of the chi-square distribution of the test's degrees
    of freedom, so a correct rule fails once in a million seeds and a wrong distribution (a wrong temperature, a
    biased uniform) lands far beyond it."""
    V, T, N = 50, 0.8, 20000
    l = np.random.default_rng(7).normal(0, 2.5, V).astype(np.float32)
    q = np.exp((l.astype(np.float64) - l.max()) / T)
    q /= q.sum()
    counts = np.bincount([R.draw(l, T, 0, 1.0, 7, n & 0xFFFF, n >> 16) for n in range(N)], minlength=V)
    exp = q * N
    big = exp >= 5
    obs = np.r_[counts[big], counts[~big].sum()]
    ex = np.r_[exp[big], exp[~big].sum()]
    chi = float(((obs - ex) ** 2 / ex).sum())
    dof = obs.size - 1
    bound = R.chi2_quantile(1e-6, dof)
    print(f"chi-square {chi:.1f} on {dof} degrees of freedom, bound {bound:.1f}")
    assert chi <= bound
    # the same draws at another temperature are not softmax(l / 0.8): the test has power
    q2 = np.exp((l.astype(np.float64) - l.max()) / 1.0)
    q2 /= q2.sum()
    e2 = np.r_[(q2 * N)[big], (q2 * N)[~big].sum()]
    assert float(((obs - e2) ** 2 / e2).sum()) > bound
