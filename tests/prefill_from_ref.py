"""Python restatement of the packing rule with a start (include/sli.h at sli_prefill_pack_from), written from the
rule's text and not from the C planner, and of the argument checks of the extend calls in their documented order.

The rule: sequence s continued from position ``start`` with ``count`` tokens contributes rows for positions start ..
start + count - 2. Its first group is (s, start, min(16 - start % 16, count - 1)); every later group starts on a
16-boundary of the sequence's own positions. A count of 1 contributes nothing. The groups of the listed sequences are
concatenated in list order; 16 groups make a chunk; the last chunk takes the smallest of 32 / 64 / 128 / 256 rows that
holds its groups and is padded with nv == 0 groups that name the last real group's sequence at p0 = 0.
"""
from __future__ import annotations

import numpy as np

SIZES = (32, 64, 128, 256)
OK, ERR_ARG, ERR_RANGE = 0, 1, 3


def pack_from(starts, counts, seqs=None):
    """(groups [n, 3] int32 of (seq, p0, nv), padding included; chunk_rows [c] int32)."""
    counts = [int(n) for n in counts]
    starts = [int(s) for s in starts]
    seqs = list(range(len(counts))) if seqs is None else [int(s) for s in seqs]
    groups = []
    for s, st, n in zip(seqs, starts, counts):
        left = n - 1  # rows still to place
        p = st
        if left > 0:
            nv = min(16 - p % 16, left)
            groups.append((s, p, nv))
            p += nv
            left -= nv
        while left > 0:
            assert p % 16 == 0
            nv = min(16, left)
            groups.append((s, p, nv))
            p += nv
            left -= nv
    real = len(groups)
    chunk_rows = []
    for g0 in range(0, real, 16):
        need = 16 * min(16, real - g0)
        chunk_rows.append(next(m for m in SIZES if m >= need))
    if real:
        total = 16 * (len(chunk_rows) - 1) + chunk_rows[-1] // 16
        groups += [(groups[real - 1][0], 0, 0)] * (total - real)
    return np.array(groups, np.int32).reshape(-1, 3), np.array(chunk_rows, np.int32)


def extend_args(batch, max_len, vocab, pos, seqs, tokens, starts, counts, ld):
    """The status sli_model_extend_seqs gives these arguments on a model whose sequences stand at ``pos``: each
    condition of the table over every listed sequence before the next condition. tokens is [n_seqs][ld]."""
    n = len(seqs)
    if not 1 <= n <= batch:
        return ERR_ARG
    for i, s in enumerate(seqs):
        if not 0 <= s < batch or s in list(seqs[:i]):
            return ERR_ARG
    st = [int(pos[s]) for s in seqs] if starts is None else [int(v) for v in starts]
    if any(not 1 <= c <= ld for c in counts):
        return ERR_RANGE
    if any(a + c > max_len for a, c in zip(st, counts)):
        return ERR_RANGE
    if any(not 0 <= int(t) < vocab for i, c in enumerate(counts) for t in tokens[i][:c]):
        return ERR_RANGE
    if any(not 0 <= a <= pos[s] for a, s in zip(st, seqs)):
        return ERR_RANGE
    return OK
