"""tests/attn_ref.py against the C oracle, its split form against its whole form, and the builders' claims: what the GPU
file compares the attention kernels with is checked here first, without a GPU."""
import numpy as np
import pytest

import oracle as O
from tests import attn_ref as R
from tests import gemv_ref as G

PLAN = dict(kernel=0, g=2, kv_group=1, waves=16, ppwg=64, max_splits=3, tpw=0, nbuf=0, grid=0, merge_grid=0, merge=2)
CASES = [(1, 4, 2, 64, 40, [39]), (3, 4, 4, 64, 150, [0, 149, 64]), (2, 8, 2, 128, 130, [63, 129])]


def _inputs(B, hq, hkv, hd, T, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal(B * hq * hd).astype(np.float32), r.standard_normal((B * hkv, T, hd)).astype(np.float32),
            r.standard_normal((B * hkv, T, hd)).astype(np.float32))


@pytest.mark.parametrize("B,hq,hkv,hd,T,pos", CASES)
def test_decode_against_the_oracle(B, hq, hkv, hd, T, pos):
    q, K, V = _inputs(B, hq, hkv, hd, T, 1)
    got = R.decode(q, K.astype(np.float64), V.astype(np.float64), pos, hq, hkv, hd).reshape(B, hq * hd)
    for b in range(B):  # the oracle's cache is the reference layout [L][T][hkv hd]
        kc = np.ascontiguousarray(K[b * hkv:(b + 1) * hkv].transpose(1, 0, 2)).reshape(1, T, hkv * hd)
        vc = np.ascontiguousarray(V[b * hkv:(b + 1) * hkv].transpose(1, 0, 2)).reshape(1, T, hkv * hd)
        ref = O.mha(q.reshape(B, -1)[b], kc, vc, 0, pos[b], T, hd, hq, hkv)
        np.testing.assert_allclose(got[b], ref, rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("B,hq,hkv,hd,T,pos", CASES)
def test_splits_merge_to_the_whole(B, hq, hkv, hd, T, pos):
    q, K, V = _inputs(B, hq, hkv, hd, T, 2)
    q *= 4  # (split maxima well apart)
    K, V = K.astype(np.float64), V.astype(np.float64)
    ppwg, ms = PLAN["ppwg"], PLAN["max_splits"]
    states = [R.split_state(q, K, V, pos, hq, hkv, hd, ppwg, s) for s in range(ms)]
    ns = R.ns_of_heads(pos, hq, PLAN)
    for s, (m, lse, on) in enumerate(states):  # dead exactly where the sequence does not reach
        assert np.array_equal(np.isnan(m), ns <= s) and (lse[ns > s] >= m[ns > s]).all()
    merged = R.merge_heads(R.part_of_states(states, hd, ms), ns, hd)
    np.testing.assert_allclose(merged, R.decode(q, K, V, pos, hq, hkv, hd), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("kv", ("f32", "f16", "f8"))
def test_needle(kv):
    hits = {}
    pos = [100, 0, 149]
    q, Kc, Vc, want = R.needle(pos, 4, 2, 64, 150, kv, PLAN, 3, hits)
    K, V = R.values(Kc, kv), R.values(Vc, kv)
    sc = R.scores(q, K, pos, 4, 2, 64)
    for s in sc:  # one needle at 4096 / sqrt(hd), everything else 0
        assert np.sort(s)[-1] == 4096 / 8 and (np.sort(s)[:-1] == 0).all()
    assert np.float32(np.exp(np.float32(-362.0))) == 0  # every other weight is exactly 0 in fp32
    live = [K[h, :pos[h // 2] + 1] for h in range(6)]
    assert all(np.isfinite(x).all() for x in live)
    np.testing.assert_array_equal(R.decode(q, _live(K, pos, 2), _live(V, pos, 2), pos, 4, 2, 64), want)
    assert (want != 0).all() and sum(hits.values()) == 12
    # the rows past pos hold the poison, +- alternating
    if kv != "f8":
        assert np.abs(K[0, 101:]).min() == float(np.float32(R.POISON[kv])) and (K[0, 101:] > 0).any() and (K[0, 101:] < 0).any()
    else:
        assert set(np.unique(Kc[0, 101:])) == {0x7E, 0xFE}


def _live(X, pos, hkv):
    """X with the rows past pos zeroed (0 * poison would be NaN in a float64 product that the mask discards)."""
    X = X.copy()
    for kvh in range(X.shape[0]):
        X[kvh, pos[kvh // hkv] + 1:] = 0
    return X


def test_needle_rows():
    rows = R.needle_rows(149, PLAN)  # slices of 4 rows, tiles of 32, splits of 64
    assert rows == dict(row0=0, pos=149, slice_first=148, slice_last=147, tile_first=128, tile_last=127, split_first=128,
                        split_last=127)
    assert R.needle_rows(3, PLAN) == dict(row0=0, pos=3)
    assert R.needle_rows(32, dict(PLAN, kernel=1)) == dict(row0=0, pos=32, slice_first=32, slice_last=31, tile_first=32,
                                                           tile_last=31)


@pytest.mark.parametrize("kv", ("f32", "f16", "f8"))
def test_uniform(kv):
    pos = [31, 77]
    q, Kc, Vc, V = R.uniform(pos, 4, 2, 64, 150, kv, 4)
    assert not R.values(Kc, kv)[0, :32].any() and np.array_equal(R.values(Vc, kv)[2, :78], V[2, :78])
    ref = R.decode(q, _live(R.values(Kc, kv), pos, 2), _live(V, pos, 2), pos, 4, 2, 64).reshape(2, 4, 64)
    np.testing.assert_allclose(ref[0, 0], V[0, :32].sum(axis=0) / 32, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(ref[1, 3], V[3, :78].sum(axis=0) / 78, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("kv", ("f32", "f16", "f8"))
def test_realistic(kv):
    pos = [149, 20, 64]
    plan = dict(PLAN, kernel=1, waves=4)
    q, Kc, Vc, scaled = R.realistic(pos, 4, 2, 64, 150, kv, plan, 5)
    assert scaled.tolist() == [False, True] * 6
    K, V = _live(R.values(Kc, kv), pos, 2), _live(R.values(Vc, kv), pos, 2)
    ns = R.ns_of_heads(pos, 4, plan)
    assert ns.tolist() == [3] * 4 + [1] * 4 + [2] * 4
    tol, tol_lse = R.real_tol(q, K, V, pos, 4, 2, 64, ns)
    tol = tol.reshape(12, 64)
    t1, l1 = R.real_tol(q, K, V, pos, 4, 2, 64, ns, split=(64, 1))
    assert np.array_equal(np.isnan(l1), ns <= 1) and np.isfinite(tol_lse).all() and (l1[ns > 1] < 1e-2).all()
    ref = R.decode(q, K, V, pos, 4, 2, 64).reshape(12, 64)
    assert np.isfinite(tol).all() and (tol > 0).all()
    # the bound is meaningful: well below the values it guards, and looser than the fp32 rounding of the result
    assert np.median(tol[scaled] / np.abs(ref[scaled])) < 1e-2 and (tol >= R.U32 * np.abs(ref)).all()
    # a merge that took its maximum from split 0 would overflow: the weight of a later split is e^(>= 120)
    sc = R.scores(q, K, pos, 4, 2, 64)
    with np.errstate(over="ignore"):
        assert sc[1].max() - sc[1][:64].max() >= 120 and np.exp(np.float32(120)) == np.float32(np.inf)


def test_positions_and_the_position_array():
    plan = dict(PLAN, ppwg=128, waves=16, max_splits=4)
    ps = R.positions(plan, 500)
    assert ps[0] == 499 and set(ps) >= {0, 7, 8, 31, 32, 127, 128, 499}
    odd = [p for p in ps if p > 384 and p < 499][0]
    assert (odd - 384) % 32 not in (0, 31) and (odd - 384) // 8 < 15  # a masked tail inside a tile, dead waves behind it
    sets = R.pos_sets(plan, 500, 4, 3, special=True)
    assert sets[0][:3] == [499, 0, 499] and all(len(set(v)) == 4 for v in sets[1:])
    a = R.pos_array([5, 6, 7])
    assert a[0] == 5 and a[6] == 6 and a[12] == 7 and (np.delete(a, [0, 6, 12]) == R.POS_POISON).all()
    assert G.live_splits(127, 128, 4) == 1 and G.live_splits(128, 128, 4) == 2


def test_f8_encode_is_the_table_search():
    from tests import kv8_ref as F8
    r = np.random.default_rng(6)
    x = np.concatenate([r.standard_normal(20000) * 10.0 ** r.integers(-4, 3, 20000), F8.MAGS, -F8.MAGS, F8.MIDS, -F8.MIDS,
                        np.nextafter(F8.MIDS.astype(np.float32), np.float32(0)), [0.0, -0.0, 448.0, 449.0, 1e9, -1e9,
                                                                                 np.inf, -np.inf]]).astype(np.float32)
    assert np.array_equal(R.f8_encode(x), F8.encode(x))
    assert R.f8_encode(np.array([np.nan], np.float32))[0] == 0x7F


def test_production_merge_rule():
    assert R.production_merge("f16", 128, 2048, 1) == 1 and R.production_merge("f16", 128, 4096, 1) == 0
    assert R.production_merge("f32", 128, 2048, 1) == 0 and R.production_merge("f8", 128, 2048, 1) == 0
    assert R.production_merge("f16", 128, 2048, 8) == 2
