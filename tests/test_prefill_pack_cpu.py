"""The packing rule of the batched prompt prefill (sli_prefill_pack, host only) against its numpy restatement
(tests/prefill_pack_ref.py) and against the invariants the kernels rely on. No GPU."""
import ctypes

import numpy as np
import pytest

from tests import prefill_pack_ref as P

SIZES = (32, 64, 128, 256)


def _pack(lens, seqs=None):
    from simplellminference_amd import ops
    return ops.prefill_pack(lens, seqs)


def _cases(n=300):
    r = np.random.default_rng(2024)
    for i in range(n):
        k = int(r.integers(1, 9))
        seqs = r.permutation(8)[:k]
        hi = (600, 40, 3)[i % 3]  # long prompts, short ones, and mostly lengths 1 and 2
        yield seqs.astype(np.int32), r.integers(1, hi + 1, k).astype(np.int32)


def test_planner_equals_the_restatement():
    n = 0
    for seqs, lens in _cases():
        g, rows = _pack(lens, seqs)
        rg, rrows = P.pack(lens, seqs)
        assert np.array_equal(rows, rrows), (seqs, lens, rows, rrows)
        assert np.array_equal(g, rg), (seqs, lens)
        n += 1
    assert n >= 300


def test_invariants_of_the_planner_output():
    for seqs, lens in _cases():
        g, rows = _pack(lens, seqs)
        real = g[g[:, 2] > 0]
        # every (seq, position < len - 1) exactly once
        want = sorted((int(s), p) for s, n in zip(seqs, lens) for p in range(n - 1))
        got = sorted((int(s), int(p0) + r) for s, p0, nv in real for r in range(nv))
        assert got == want
        assert np.all(g[:, 1] % 16 == 0) and np.all((g[:, 2] >= 0) & (g[:, 2] <= 16))
        # list order, and a sequence's groups ascend: the real groups are exactly this sequence of (seq, p0)
        order = [(int(s), p0) for s, n in zip(seqs, lens) for p0 in range(0, n - 1, 16)]
        assert [(int(s), int(p0)) for s, p0, _ in real] == order
        # only a sequence's last group may be partial
        for s, n in zip(seqs, lens):
            nv = g[(g[:, 0] == s) & (g[:, 2] > 0)][:, 2]
            assert np.all(nv[:-1] == 16)
            if n > 1:
                assert nv[-1] == ((n - 1) % 16 or 16)
        # chunks
        assert len(rows) == -(-len(real) // 16)
        assert np.all(rows[:-1] == 256)
        if len(rows):
            need = 16 * (len(real) - 16 * (len(rows) - 1))
            assert rows[-1] == min(m for m in SIZES if m >= need)
            assert len(g) == 16 * (len(rows) - 1) + rows[-1] // 16
        # padding only at the end of the last chunk
        assert np.all(g[:len(real), 2] > 0) and np.all(g[len(real):, 2] == 0)
        assert len(g) - len(real) < 16
        assert set(g[:, 0].tolist()) <= set(seqs.tolist())


def test_edge_cases():
    g, rows = _pack([1, 1, 1, 1])
    assert len(g) == 0 and len(rows) == 0
    g, rows = _pack([17])
    assert rows.tolist() == [32] and g.tolist() == [[0, 0, 16], [0, 0, 0]]
    g, rows = _pack([257], seqs=[5])
    assert rows.tolist() == [256] and g[:, 2].tolist() == [16] * 16 and g[:, 1].tolist() == list(range(0, 256, 16))
    assert set(g[:, 0].tolist()) == {5}
    g, rows = _pack([258], seqs=[5])
    assert rows.tolist() == [256, 32]
    assert g[16].tolist() == [5, 256, 1] and g[17].tolist() == [5, 0, 0] and len(g) == 18
    g, rows = _pack([2, 34])  # one row of sequence 0, then 33 of sequence 1: 4 groups
    assert rows.tolist() == [64] and g.tolist() == [[0, 0, 1], [1, 0, 16], [1, 16, 16], [1, 32, 1]]


def test_one_sequence_plan_is_the_batch_1_chunk_rule():
    """sli_model_prefill and sli_tp_group_prefill run the plan of the one sequence 0. It is the chunking they always had:
    chunks of up to 256 consecutive positions from 0, each the smallest size that holds its rows, the real groups the
    16-row runs of positions 0 .. n - 2 in order."""
    for n in range(1, 1101):
        g, rows = _pack([n], [0])
        old = [min(m for m in SIZES if m >= min(256, n - 1 - p0)) for p0 in range(0, n - 1, 256)]
        assert rows.tolist() == old, n
        real = [tuple(r) for r in g.tolist() if r[2] > 0]
        assert real == [(0, 16 * k, min(16, n - 1 - 16 * k)) for k in range(-(-(n - 1) // 16))], n


def test_refusals():
    from simplellminference_amd import _lib
    from simplellminference_amd._lib import SliError

    def raw(lens, cap_g, cap_c):
        lens = np.asarray(lens, np.int32)
        seqs = np.arange(lens.size, dtype=np.int32)
        g = np.zeros((max(cap_g, 1), 3), np.int32)
        rows = np.zeros(max(cap_c, 1), np.int32)
        n = ctypes.c_int32(-1)
        _lib.call("sli_prefill_pack", seqs.ctypes.data_as(ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p),
                  lens.size, g.ctypes.data_as(ctypes.c_void_p), cap_g, rows.ctypes.data_as(ctypes.c_void_p), cap_c,
                  ctypes.byref(n))
        return n.value

    assert raw([40, 300], 32, 2) == 2      # 3 + 19 groups: 16 + 6 -> a 256-row and a 128-row chunk = 24 groups
    for cap_g, cap_c in ((23, 2), (24, 1)):
        with pytest.raises(SliError) as e:
            raw([40, 300], cap_g, cap_c)
        assert e.value.code == 3, e.value  # SLI_ERR_RANGE
    for lens in ([0], [5, 0, 7], [-3]):
        with pytest.raises(SliError) as e:
            raw(lens, 64, 8)
        assert e.value.code == 3, e.value
