"""tests/gen_ref.py against hand-computed cases and against itself: the penalty rule element by element, the window,
out-of-range history entries, an fp32 stand-in implementation accepted on random rows with mixed settings, and the
neutral block reproducing tests/sample_ref.py's draw."""
import numpy as np

from tests import gen_ref as G
from tests import sample_ref as R

F = np.float32


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_penalty_hand_cases():
    # index:        0     1     2     3      4       5      6     7
    l = np.array([2.0, -2.0, 0.0, -0.0, np.nan, -np.inf, 3.0, -1.5], np.float32)
    hist = [0, 1, 2, 3, 4, 5, 0, 0]  # token 0 three times, tokens 1..5 once, 6 and 7 never
    P = G.params(repetition_penalty=2.0, presence_penalty=0.5, frequency_penalty=0.25)
    out = G.penalise(l, hist, 7, P)
    assert out[0] == F(2.0 / 2.0 - 0.5 - 0.25 * 3) == F(-0.25)       # positive, count 3: divided
    assert out[1] == F(-2.0 * 2.0 - 0.5 - 0.25) == F(-4.75)          # negative, count 1: multiplied
    assert out[2] == F(-0.75) and out[3] == F(-0.75)                 # +-0 take the multiply branch: +-0 * 2 - 0.5 - 0.25
    assert np.isnan(out[4])                                          # a NaN stays a NaN
    assert out[5] == -np.inf                                         # -inf * 2 - ... = -inf
    assert _bits(out[6:]).tolist() == _bits(l[6:]).tolist()          # count 0: bit for bit
    # repetition alone keeps the sign of zero (the multiply branch), and count 0 keeps -0
    only_rp = G.penalise(l, hist, 7, G.params(repetition_penalty=1.5))
    assert _bits(only_rp[2:4]).tolist() == _bits([0.0, -0.0]).tolist()
    assert only_rp[0] == F(F(2.0) / F(1.5)) and only_rp[1] == F(-3.0)
    # each operation rounds once: a value where (l / rp) - pp differs from a fused or double evaluation
    l2 = np.array([1.0], np.float32)
    P2 = G.params(repetition_penalty=3.0, presence_penalty=1e-8, frequency_penalty=1e-8)
    a = F(F(1.0) / F(3.0))
    want = F(F(a - F(1e-8)) - F(F(1e-8) * F(1.0)))
    assert _bits(G.penalise(l2, [0], 0, P2))[0] == _bits(want)


def test_penalty_inactive_is_the_row_itself():
    l = np.array([1.0, np.nan, -0.0, 5.0], np.float32)
    out = G.penalise(l, [0, 0, 3], 2, G.params(temperature=1.0, min_p=0.3))
    assert _bits(out).tolist() == _bits(l).tolist()


def test_penalty_window():
    V = 6
    l = np.arange(1, V + 1, dtype=np.float32)
    hist = [0, 1, 2, 3, 4, 5]
    for frm, pos, hit in ((0, 5, [0, 1, 2, 3, 4, 5]), (0, 2, [0, 1, 2]), (3, 5, [3, 4, 5]), (4, 4, [4]), (5, 4, []),
                          (100, 5, [])):
        out = G.penalise(l, hist, pos, G.params(presence_penalty=1.0, penalty_from=frm))
        assert np.flatnonzero(out != l).tolist() == hit, (frm, pos)
        assert G.counts(hist, pos, G.params(penalty_from=frm), V).sum() == len(hit)


def test_history_entries_outside_the_vocabulary_are_not_counted():
    V = 4
    l = np.ones(V, np.float32)
    hist = [-1, 4, 2, 2 ** 31 - 1, -2 ** 31, 1000, 2]
    P = G.params(frequency_penalty=0.5)
    assert G.counts(hist, 6, P, V).tolist() == [0, 0, 2, 0]
    assert G.penalise(l, hist, 6, P).tolist() == [1.0, 1.0, 0.0, 1.0]


def test_greedy_rows_and_min_p():
    l = np.array([1.0, 3.0, 3.0, 2.9, np.nan, -np.inf], np.float32)
    assert G.draw(l, [], 0, G.params(), 0) == 1
    assert G.draw(l, [1], 0, G.params(presence_penalty=1.0), 0) == 2  # the first maximum moves once 1 is penalised
    P = G.params(temperature=1.0, min_p=0.9)  # log(0.9) = -0.105: 2.9 passes (-0.1), 1.0 does not
    assert G.min_p_set(l, P).tolist() == [False, True, True, True, False, False]
    P = G.params(temperature=1.0, min_p=np.nextafter(F(1), F(0)))  # only ties with the maximum
    assert G.min_p_set(l, P).tolist() == [False, True, True, False, False, False]
    assert G.min_p_set(np.full(7, 1.25, np.float32), P).all()


def _random_case(rng, i):
    V = int(rng.choice([1, 2, 17, 64, 300, 1000]))
    l = rng.normal(0, 2.5, V).astype(np.float32)
    if V >= 8:
        l[V // 3:V // 3 + 4] = l[V // 3]
        if i % 5 == 0:
            l[rng.integers(0, V, 3)] = [np.nan, -np.inf, -0.0]
    n = int(rng.choice([1, 2, 40, 200]))
    hist = rng.integers(-2, V + 2, n)
    if i % 3 == 0:
        hist[:] = hist[0]
    pos = int(rng.integers(0, n))
    P = G.params(temperature=float(rng.choice([0.0, 0.05, 0.7, 1.0, 2.0])), top_k=int(rng.choice([0, 1, 5, V, V + 3])),
                 top_p=float(rng.choice([1.0, 0.9, 0.3])), seed=int(rng.integers(0, 2 ** 32)),
                 min_p=float(rng.choice([0.0, 0.05, 0.5])), repetition_penalty=float(rng.choice([1.0, 1.3, 0.5])),
                 presence_penalty=float(rng.choice([0.0, 0.7, -0.4])),
                 frequency_penalty=float(rng.choice([0.0, 0.2, -0.1])), penalty_from=int(rng.integers(0, n + 1)))
    return l, hist, pos, P


def test_fp32_stand_in_is_accepted():
    rng = np.random.default_rng(11)
    sampled = 0
    for i in range(240):
        l, hist, pos, P = _random_case(rng, i)
        t = G.draw_fp32(l, hist, pos, P, seq=i % 7)
        ok, why = G.accept(t, l, hist, pos, P, seq=i % 7)
        assert ok, (i, P, why)
        sampled += P["temperature"] != 0.0
        # a token outside the sets is refused: the worst penalised logit, where the best is far above it
        lp = G.penalise(l, hist, pos, P)
        if P["temperature"] == 0.0 and l.size > 1 and np.isfinite(lp).all() and lp.max() > lp.min():
            assert not G.accept(int(np.argmin(lp)), l, hist, pos, P, seq=i % 7)[0]
    assert sampled >= 150


def test_neutral_block_is_sample_ref():
    rng = np.random.default_rng(12)
    for i in range(60):
        V = int(rng.choice([1, 5, 64, 1000]))
        l = rng.normal(0, 2.5, V).astype(np.float32)
        T, k, p, seed = float(rng.choice([0.3, 1.0, 1.7])), int(rng.choice([0, 3, V])), float(rng.choice([1.0, 0.8])), i
        P = G.params(temperature=T, top_k=k, top_p=p, seed=seed)
        hist = rng.integers(0, V, 10)
        assert G.draw(l, hist, 9, P, seq=3) == R.draw(l, T, k, p, seed, 3, 9)
        assert G.draw_fp32(l, hist, 9, P, seq=3) == R.draw_fp32(l, T, k, p, seed, 3, 9)
        ok, _ = G.accept(R.draw(l, T, k, p, seed, 3, 9), l, hist, 9, P, seq=3)
        assert ok
