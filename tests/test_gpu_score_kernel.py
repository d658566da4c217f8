"""score_rows_kernel (csrc/score.h) through ops.score_rows against the float64 rule (tests/score_ref.py) on the same
fp32 logits.

Bar: top exact; |d logprob| and |d top_logprob| <= 2e-5, derived, not tuned: S = sum exp(l_j - M) >= 1; each term
carries expf's few-ulp error plus |l_j - M| 2^-24 from the subtraction, weighted by a term <= 1/e; a per-thread chain
of <= 126 additions plus a <= 10-level merge gives <= ~140 2^-24 ~ 8e-6 relative on S, the same absolute error on
log S; forming M + log S (|lse| < 42) and the final subtraction add <= 5e-6: worst case ~1.5e-5, rounded up. (That
is the count for 256 threads a row; the kernel's 1024 threads make the chain <= 32 additions, a 6-level wave tree and
15 merges in wave order, fewer roundings under the same bar.) Measured on an MI355X: at most 3.7e-6 / 2.1e-6 at
256 x 128 256 and 1.9e-6 at the smaller shapes.

Rows: N(0, sigma^2) with sigma 1 and 8 in turn, clipped to |l| <= 30, and five special rows (one logit 30 above the
rest; all equal; some -inf; the maximum twice, at V - 1 and 3; +0 / -0 tied for the top); targets at 0, at V - 1, at
the top and at random; one target equal to V on a row that is not the launch's last. Shapes with fewer than eight rows
run as many calls as it takes to place every kind of row and target.
"""
import numpy as np
import pytest

from tests import score_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16), (3, 17), (16, 512), (32, 1000), (5, 32000), (256, 128256)]
TOL = 2e-5
KINDS = 8  # 0 .. 4: the special rows; 5 .. 7: plain


def _row(rng, V, kind, sigma):
    l = np.clip(rng.normal(0.0, sigma, V), -30, 30).astype(np.float32)
    if kind == 0:  # one logit 30 above the rest
        l = -np.abs(l)
        l[V // 2] = l.max() + np.float32(30)
    elif kind == 1:
        l[:] = np.float32(1.25)
    elif kind == 2:
        l[rng.random(V) < 0.125] = -np.inf
        l[V // 3] = np.float32(0.5)  # (at least one finite logit)
    elif kind == 3:
        l = np.minimum(l, np.float32(29))
        l[V - 1] = l[3] = l.max() + np.float32(1)
    elif kind == 4:
        l = -np.abs(l) - np.float32(1e-3)
        l[5], l[9] = np.float32(-0.0), np.float32(0.0)
    return l


def _case(M, V, call, seed):
    rng = np.random.default_rng(seed)
    L = np.empty((M, V), np.float32)
    t = np.empty(M, np.int32)
    for m in range(M):
        k = call * M + m
        L[m] = _row(rng, V, k % KINDS, (1.0, 8.0)[m % 2])
        mode = (k // KINDS + k) % 4
        t[m] = (0, V - 1, R.first_max(L[m]), int(rng.integers(0, V)))[mode]
    if M >= 2:
        t[(M - 1) // 2] = V  # out of range, and not the launch's last row
    return L, t


def _run(torch, L, t, ld=None):
    from simplellminference_amd import ops
    M, V = L.shape
    if ld is None:
        dl = torch.from_numpy(L).cuda()
    else:  # rows ld floats apart, the padding columns 1e30
        buf = torch.full((M, ld), 1e30, dtype=torch.float32, device="cuda")
        buf[:, :V] = torch.from_numpy(L).cuda()
        dl = buf[:, :V]
    lp, top, tlp = ops.score_rows(dl, torch.from_numpy(t).cuda())
    torch.cuda.synchronize()
    return lp.cpu().numpy(), top.cpu().numpy(), tlp.cpu().numpy()


def _hold(L, t, got):
    lp, top, tlp = got
    rlp, rtop, rtlp = R.score_rows(L, t)
    assert np.array_equal(top, rtop), np.nonzero(top != rtop)
    oor = (t < 0) | (t >= L.shape[1])
    assert np.isnan(lp[oor]).all() and np.isnan(rlp[oor]).all()
    inf = np.isneginf(rlp)  # a -inf target
    assert np.array_equal(np.isneginf(lp), inf)
    ok = ~oor & ~inf
    e1 = float(np.abs(lp[ok] - rlp[ok]).max()) if ok.any() else 0.0
    e2 = float(np.abs(tlp - rtlp).max())
    assert np.isfinite(tlp).all()
    return e1, e2


@pytest.fixture(scope="module")
def big(gpu):
    M, V = SHAPES[-1]
    L, t = _case(M, V, 0, 5)
    return L, t, _run(gpu, L, t)


@pytest.mark.parametrize("M,V", SHAPES[:-1])
def test_rows_match_the_rule(gpu, M, V):
    worst = (0.0, 0.0)
    for call in range(-(-KINDS // M) if M < KINDS else 1):
        L, t = _case(M, V, call, 100 * M + call)
        worst = tuple(max(a, b) for a, b in zip(worst, _hold(L, t, _run(gpu, L, t))))
    print(f"M {M} V {V}: max|d logprob| {worst[0]:.3e}, max|d top_logprob| {worst[1]:.3e}")
    assert worst[0] <= TOL and worst[1] <= TOL, worst


def test_rows_match_the_rule_at_the_llama3_vocabulary(gpu, big):
    L, t, got = big
    e1, e2 = _hold(L, t, got)
    print(f"M {L.shape[0]} V {L.shape[1]}: max|d logprob| {e1:.3e}, max|d top_logprob| {e2:.3e}")
    assert e1 <= TOL and e2 <= TOL, (e1, e2)


def test_special_rows_give_what_the_rule_says(gpu):
    V = 1000
    L, t = _case(8, V, 0, 9)
    lp, top, tlp = _run(gpu, L, t)
    assert top[0] == V // 2 and abs(tlp[0]) <= TOL            # the spike holds all the mass but ~V e^-30
    assert top[1] == 0 and abs(tlp[1] + np.log(V)) <= TOL     # all equal: -ln V
    assert top[3] == 3 and top[4] == 5
    assert np.isnan(lp[3]) and t[3] == V                      # the out-of-range target (row (M - 1) // 2)
    assert not np.isnan(lp[np.arange(8) != 3]).any()


@pytest.mark.parametrize("M,V", [(3, 17), (32, 1000)])
def test_padding_columns_change_nothing(gpu, M, V):
    L, t = _case(M, V, 0, 3)
    a = _run(gpu, L, t)
    b = _run(gpu, L, t, ld=(V + 3) // 4 * 4 + 4)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_two_runs_are_bit_equal_and_a_row_does_not_depend_on_its_launch(gpu, big):
    L, t, got = big
    again = _run(gpu, L, t)
    for x, y in zip(got, again):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for m in (0, 37, 255):
        alone = _run(gpu, L[m:m + 1], t[m:m + 1])
        for x, y in zip(got, alone):
            assert np.array_equal(x[m:m + 1].view(np.uint32), y.view(np.uint32)), m
