"""numpy restatement of the scoring rule of include/sli.h (sli_score_rows), in float64 from the fp32 logits:

    lse = M + log(sum_j exp(l_j - M)), M = max_j l_j;  logprob = l_t - lse;
    top = the first index of the maximum in sli_argmax's order;  top_logprob = l_top - lse.

-inf logits contribute 0; a target outside [0, V) gives NaN; a row with a NaN logit gives NaN log-probabilities.
Restated from the header's text, not from the kernel.
"""
from __future__ import annotations

import numpy as np


def first_max(l):
    """sli_argmax: std::max_element's scan `if (*best < *it) best = it` (the first maximum; -0 equals +0; a NaN never
    displaces the best so far and, at index 0, is never displaced)."""
    l = np.asarray(l, np.float32)
    if np.isnan(l[0]):
        return 0
    x = np.where(np.isnan(l), -np.inf, l.astype(np.float64))
    return int(np.argmax(x))  # the first index of the maximum; -0.0 == +0.0


def first_max_scan(l):
    """The scan itself, element by element (what first_max is checked against)."""
    best = 0
    for i in range(1, len(l)):
        if l[best] < l[i]:
            best = i
    return best


def lse(l):
    l = np.asarray(l, np.float32).astype(np.float64)
    if np.isnan(l).any():
        return np.nan
    m = l.max()
    if not np.isfinite(m):
        return np.nan if m > 0 else -np.inf  # a +inf: inf - inf; nothing but -inf: log 0
    return m + np.log(np.exp(l - m).sum())


def score_row(l, target):
    """(logprob, top, top_logprob) of one row, float64."""
    l = np.asarray(l, np.float32)
    z = lse(l)
    top = first_max(l)
    with np.errstate(invalid="ignore"):
        lp = float(l[target]) - z if 0 <= target < len(l) else np.nan
        return lp, top, float(l[top]) - z


def score_rows(logits, targets):
    """Rows of a [M, V] array: logprob [M] float64, top [M] int32, top_logprob [M] float64."""
    logits = np.asarray(logits, np.float32)
    r = [score_row(logits[m], int(targets[m])) for m in range(logits.shape[0])]
    return (np.array([x[0] for x in r], np.float64), np.array([x[1] for x in r], np.int32),
            np.array([x[2] for x in r], np.float64))


def top2_gap(l):
    """The gap between the largest and the second largest logit of a row (0 for a tie), float64."""
    s = np.sort(np.asarray(l, np.float32).astype(np.float64))
    return float(s[-1] - s[-2])
