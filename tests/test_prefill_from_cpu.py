"""The packing rule with a start (sli_prefill_pack_from, host only) against its Python restatement
(tests/prefill_from_ref.py), against sli_prefill_pack at start 0 and against the invariants the kernels rely on; and
the argument checks of the extend calls through their host-only hook (sli_debug_extend_seqs_args). No GPU."""
import ctypes

import numpy as np
import pytest

from tests import prefill_from_ref as F

SIZES = (32, 64, 128, 256)


def _pack_from(starts, counts, seqs=None):
    from simplellminference_amd import ops
    return ops.prefill_pack_from(starts, counts, seqs)


def _cases(n=360):
    r = np.random.default_rng(7)
    edge_starts = (0, 15, 16, 17, 31, 32, 33, 47)
    edge_counts = (1, 2, 17)
    for i in range(n):
        k = int(r.integers(1, 9))
        seqs = r.permutation(8)[:k].astype(np.int32)
        hi = (600, 40, 3)[i % 3]  # long continuations (several chunks), short ones, mostly counts 1 and 2
        counts = r.integers(1, hi + 1, k)
        starts = r.integers(0, 200, k)
        if i % 2:  # the starts at 0, 15, 16 and 17 mod 16 and the counts 1, 2 and 17, in every combination over the run
            starts[0] = edge_starts[(i // 2) % len(edge_starts)]
            counts[0] = edge_counts[(i // 16) % len(edge_counts)]
        yield seqs, starts.astype(np.int32), counts.astype(np.int32)


def test_planner_equals_the_restatement():
    n = multi = 0
    seen = set()
    for seqs, starts, counts in _cases():
        g, rows = _pack_from(starts, counts, seqs)
        rg, rrows = F.pack_from(starts, counts, seqs)
        assert np.array_equal(rows, rrows), (seqs, starts, counts, rows, rrows)
        assert np.array_equal(g, rg), (seqs, starts, counts)
        n += 1
        multi += len(rows) > 1
        seen |= {(int(s) % 16, int(c)) for s, c in zip(starts, counts)}
    assert n >= 300 and multi >= 50
    assert {(s, c) for s in (0, 15, 1) for c in (1, 2, 17)} <= seen  # 0, 15, 16 (= 0) and 17 (= 1) mod 16


def test_start_zero_is_the_from_zero_planner_entry_for_entry():
    from simplellminference_amd import ops
    r = np.random.default_rng(11)
    for i in range(300):
        k = int(r.integers(1, 9))
        seqs = r.permutation(8)[:k].astype(np.int32)
        lens = r.integers(1, (600, 40, 3)[i % 3] + 1, k).astype(np.int32)
        g0, rows0 = ops.prefill_pack(lens, seqs)
        g1, rows1 = _pack_from(np.zeros(k, np.int32), lens, seqs)
        assert np.array_equal(g0, g1) and np.array_equal(rows0, rows1), (seqs, lens)


def test_invariants_of_the_planner_output():
    for seqs, starts, counts in _cases():
        g, rows = _pack_from(starts, counts, seqs)
        real = g[g[:, 2] > 0]
        # every row of the plan exactly once: (seq, position) for positions start .. start + count - 2
        want = sorted((int(s), p) for s, a, n in zip(seqs, starts, counts) for p in range(a, a + n - 1))
        got = sorted((int(s), int(p0) + r) for s, p0, nv in real for r in range(nv))
        assert got == want
        # no group crosses a 16-boundary of its sequence
        assert np.all(real[:, 1] // 16 == (real[:, 1] + real[:, 2] - 1) // 16)
        assert np.all((g[:, 2] >= 0) & (g[:, 2] <= 16))
        for s, a, n in zip(seqs, starts, counts):
            mine = real[real[:, 0] == s]
            if n == 1:
                assert len(mine) == 0
                continue
            # the first group starts at the start, every later one on a boundary, ascending and gapless
            assert mine[0, 1] == a and mine[0, 2] == min(16 - a % 16, n - 1)
            assert np.all(mine[1:, 1] % 16 == 0)
            assert np.all(mine[1:, 1] == mine[:-1, 1] + mine[:-1, 2])
            assert np.all(mine[1:-1, 2] == 16)
        # list order
        order = [int(s) for s, n in zip(seqs, counts) if n > 1]
        firsts = [int(s) for j, (s, _, _) in enumerate(real) if j == 0 or real[j - 1, 0] != s]
        assert firsts == order
        # chunks and padding
        assert len(rows) == -(-len(real) // 16)
        assert np.all(rows[:-1] == 256)
        if len(rows):
            need = 16 * (len(real) - 16 * (len(rows) - 1))
            assert rows[-1] == min(m for m in SIZES if m >= need)
            assert len(g) == 16 * (len(rows) - 1) + rows[-1] // 16
            assert np.all(g[len(real):, 0] == real[-1, 0]) and np.all(g[len(real):, 1] == 0)
        assert np.all(g[:len(real), 2] > 0) and np.all(g[len(real):, 2] == 0)


def test_edge_cases():
    g, rows = _pack_from([5, 16, 0], [1, 1, 1])
    assert len(g) == 0 and len(rows) == 0
    g, rows = _pack_from([10], [23])  # 22 rows from 10: the partial first group, then one aligned group
    assert rows.tolist() == [32] and g.tolist() == [[0, 10, 6], [0, 16, 16]]
    g, rows = _pack_from([16], [17])
    assert rows.tolist() == [32] and g.tolist() == [[0, 16, 16], [0, 0, 0]]
    g, rows = _pack_from([15], [2], seqs=[3])
    assert rows.tolist() == [32] and g.tolist() == [[3, 15, 1], [3, 0, 0]]
    g, rows = _pack_from([15], [3], seqs=[3])
    assert g.tolist() == [[3, 15, 1], [3, 16, 1]]
    g, rows = _pack_from([17], [40])  # 39 rows: 15 + 16 + 8
    assert rows.tolist() == [64] and g.tolist() == [[0, 17, 15], [0, 32, 16], [0, 48, 8], [0, 0, 0]]
    g, rows = _pack_from([35], [4])  # positions 35 .. 37
    assert g.tolist() == [[0, 35, 3], [0, 0, 0]]
    g, rows = _pack_from([8], [258], seqs=[2])  # 257 rows from 8: 8, 15 x 16, then 9 in a second chunk
    assert rows.tolist() == [256, 32] and len(g) == 18
    assert g[0].tolist() == [2, 8, 8] and g[15].tolist() == [2, 240, 16] and g[16].tolist() == [2, 256, 9]


def test_refusals_of_the_planner():
    from simplellminference_amd import _lib
    from simplellminference_amd._lib import SliError

    def raw(starts, counts, cap_g, cap_c):
        counts = np.asarray(counts, np.int32)
        starts = np.asarray(starts, np.int32)
        seqs = np.arange(counts.size, dtype=np.int32)
        g = np.zeros((max(cap_g, 1), 3), np.int32)
        rows = np.zeros(max(cap_c, 1), np.int32)
        n = ctypes.c_int32(-1)
        vp = ctypes.c_void_p
        _lib.call("sli_prefill_pack_from", seqs.ctypes.data_as(vp), starts.ctypes.data_as(vp), counts.ctypes.data_as(vp),
                  counts.size, g.ctypes.data_as(vp), cap_g, rows.ctypes.data_as(vp), cap_c, ctypes.byref(n))
        return n.value

    assert raw([8, 0], [40, 300], 32, 2) == 2  # 4 + 19 groups: 16 + 7 -> a 256-row and a 128-row chunk = 24 groups
    for cap_g, cap_c in ((23, 2), (24, 1)):
        with pytest.raises(SliError) as e:
            raw([8, 0], [40, 300], cap_g, cap_c)
        assert e.value.code == 3, e.value  # SLI_ERR_RANGE
    for starts, counts in (([0], [0]), ([0, 0, 0], [5, 0, 7]), ([-1], [4]), ([0], [-3])):
        with pytest.raises(SliError) as e:
            raw(starts, counts, 64, 8)
        assert e.value.code == 3, e.value


# ---------------------------------------------------------------- the argument checks of the extend calls
B, T, V = 4, 40, 100
POS = [0, 7, 20, 39]


def _args(seqs, tokens, starts, counts, ld=None, pos=POS, batch=B):
    """The status of sli_debug_extend_seqs_args (no exception: the codes are what is compared)."""
    from simplellminference_amd import _lib
    lib = _lib.load()
    ld = max(max(len(t) for t in tokens), 1) if ld is None else ld
    P = np.zeros((len(tokens), ld), np.int32)
    for i, t in enumerate(tokens):
        P[i, :len(t)] = t
    vp = ctypes.c_void_p
    seqs = np.asarray(seqs, np.int32)
    counts = np.asarray(counts, np.int32)
    pos = np.asarray(pos, np.int32)
    st = None if starts is None else np.asarray(starts, np.int32)
    rc = lib.sli_debug_extend_seqs_args(batch, T, V, pos.ctypes.data_as(vp), seqs.ctypes.data_as(vp), seqs.size,
                                        P.ctypes.data_as(vp), st.ctypes.data_as(vp) if st is not None else None,
                                        counts.ctypes.data_as(vp), ld)
    ref = F.extend_args(batch, T, V, pos.tolist(), seqs.tolist(), P.tolist(), None if st is None else st.tolist(),
                        counts.tolist(), ld)
    assert rc == ref, (rc, ref)
    return rc


def test_extend_args_accepts():
    assert _args([1], [[1, 2, 3]], [7], [3]) == 0           # start == pos
    assert _args([1], [[1, 2, 3]], [0], [3]) == 0           # a rollback to 0
    assert _args([1], [[1, 2, 3]], None, [3]) == 0          # NULL starts: the current position
    assert _args([2], [[5] * 20], [20], [20]) == 0          # start + count == max_len
    assert _args([3], [[5]], [39], [1]) == 0                # the last position, one token
    assert _args([0], [[5] * 40], [0], [40]) == 0           # a fresh sequence takes the whole length
    assert _args([3, 0, 2], [[1], [2, 3], [4]], [10, 0, 20], [1, 2, 1]) == 0
    assert _args([1], [[1, 2, 3]], [7], [2]) == 0           # a count below ld reads only its own tokens
    assert _args([1], [[1, 2, V]], [7], [2]) == 0


def test_extend_args_each_error_code():
    assert _args([], [[1]], [0], [1]) == 1                  # no sequence listed: SLI_ERR_ARG
    assert _args([4], [[1]], [0], [1]) == 1                 # out of range: SLI_ERR_ARG
    assert _args([-1], [[1]], [0], [1]) == 1
    assert _args([1, 1], [[1], [1]], [0, 0], [1, 1]) == 1   # listed twice
    assert _args([0, 1, 2, 3, 0], [[1]] * 5, [0] * 5, [1] * 5) == 1  # n_seqs above the batch
    assert _args([1], [[1, 2]], [0], [0]) == 3              # count below 1: SLI_ERR_RANGE
    assert _args([1], [[1, 2]], [0], [3]) == 3              # count above ld
    assert _args([2], [[5] * 21], [20], [21]) == 3          # start + count > max_len
    assert _args([3], [[5, 5]], None, [2]) == 3             # the same from the current position (39 + 2)
    assert _args([1], [[1, V]], [0], [2]) == 3              # a token outside the vocabulary
    assert _args([1], [[-1, 1]], [0], [2]) == 3
    assert _args([1], [[1, 2]], [8], [2]) == 3              # start above the position
    assert _args([1], [[1, 2]], [-1], [2]) == 3             # start below 0
    assert _args([0], [[1, 2]], [1], [2]) == 3              # a fresh sequence starts at 0 only


def test_extend_args_order():
    """The one order: sequence list (ARG) before counts, counts before start + count, that before tokens, tokens before
    the start's range. Where two conditions fail with the same code the message tells them apart."""
    from simplellminference_amd import _lib
    lib = _lib.load()

    def why():
        return lib.sli_last_error().decode()

    # a duplicate sequence AND every RANGE condition: ARG wins
    assert _args([1, 1], [[V], [V]], [30, 30], [0, 0]) == 1
    # count out of range AND start + count > max_len AND a bad token AND a bad start
    assert _args([1], [[V, V]], [39], [3]) == 3 and "count outside" in why()
    # start + count > max_len AND a bad token AND a start above the position
    assert _args([1], [[V, V]], [39], [2]) == 3 and "exceeds max_len" in why()
    # a bad token AND a start above the position
    assert _args([1], [[V, 1]], [8], [2]) == 3 and "vocab" in why()
    # the start alone
    assert _args([1], [[1, 1]], [8], [2]) == 3 and "start outside" in why()
    # a condition of a LATER sequence comes before the next condition of an earlier one
    assert _args([1, 2], [[V, 1], [1, 1]], [0, 0], [2, 3]) == 3 and "count outside" in why()
    assert _args([1, 2], [[1, 1], [V, 1]], [8, 0], [2, 2]) == 3 and "vocab" in why()


def test_entry_points_exist():
    from simplellminference_amd import _lib, ops
    from simplellminference_amd.model import LlamaModel, TPGroup
    lib = _lib.load()
    for name in ("sli_prefill_pack_from", "sli_model_extend_seqs", "sli_model_score_extend_seqs", "sli_model_extend",
                 "sli_tp_group_extend", "sli_debug_extend_seqs_args", "sli_kv_copy_prefix", "sli_model_copy_prefix",
                 "sli_tp_group_copy_prefix"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert callable(ops.prefill_pack_from) and callable(ops.kv_copy_prefix)
    for name in ("extend", "append", "score_extend", "fork", "admit"):
        assert callable(getattr(LlamaModel, name))
    assert callable(TPGroup.extend)
