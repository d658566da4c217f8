"""numpy restatement of the packing rule of the batched prompt prefill (include/sli.h at sli_prefill_pack), written
from the rule's text and not from the C planner, plus the group-table restatements of the two prefill stages that read
the table (tests/prefill_ref.py holds the per-row arithmetic; nothing here changes it).

The rule: sequence s with n prompt tokens contributes positions 0 .. n-2 in groups of 16 aligned on its own positions;
the groups of the listed sequences are concatenated in list order; 16 groups make a chunk; the last chunk takes the
smallest of 32 / 64 / 128 / 256 rows that holds its groups and is padded with nv == 0 groups.
"""
from __future__ import annotations

import numpy as np

from tests import prefill_ref as R

SIZES = (32, 64, 128, 256)


def pack(lens, seqs=None):
    """(groups [n, 3] int32 of (seq, p0, nv), padding included; chunk_rows [c] int32)."""
    lens = [int(n) for n in lens]
    seqs = list(range(len(lens))) if seqs is None else [int(s) for s in seqs]
    groups = []
    for s, n in zip(seqs, lens):
        rows = n - 1
        for p0 in range(0, rows, 16):
            groups.append((s, p0, min(16, rows - p0)))
    real = len(groups)
    chunk_rows = []
    for g0 in range(0, real, 16):
        need = 16 * min(16, real - g0)
        chunk_rows.append(next(m for m in SIZES if m >= need))
    if real:
        total = 16 * (len(chunk_rows) - 1) + chunk_rows[-1] // 16
        groups += [(groups[real - 1][0], 0, 0)] * (total - real)  # padding: the last real group's sequence, p0 0
    return np.array(groups, np.int32).reshape(-1, 3), np.array(chunk_rows, np.int32)


def epi_qkv_segs(Y, scale, sin_t, cos_t, groups, T, hq, hkv, hd):
    """The q/k/v epilogue under a group table: prefill_ref.epi_qkv per group at that group's p0. Returns q [M][hq hd]
    and a list of (seq, position, k row [hkv][hd], v row [hkv][hd]) for every row that reaches the cache."""
    M = Y.shape[0]
    q = np.empty((M, hq * hd))
    stores = []
    for g in range(M // 16):
        seq, p0, nv = (int(v) for v in groups[g]) if g < len(groups) else (0, 0, 0)
        rows = slice(16 * g, 16 * g + 16)
        qg, kg, vg, stored = R.epi_qkv(Y[rows], scale, sin_t, cos_t, p0, nv, T, hq, hkv, hd)
        q[rows] = qg
        for r in np.nonzero(stored)[0]:
            stores.append((seq, p0 + int(r), kg[r], vg[r]))
    return q, stores
