"""numpy restatement of the per-row generation rule of include/sli.h (sli_sample_gen), written from the header's text,
and the acceptance test the GPU checks use. The hash, the top-k set, the nucleus, the keys and the argmax come from
tests/sample_ref.py.

  * penalise() is in np.float32, one operation at a time: each of the rule's operations is one correctly rounded fp32
    operation, which numpy's float32 scalar arithmetic is too, so the penalised row is exact and is compared bit for
    bit wherever the draw is an argmax (temperature 0, top_k = 1).
  * C_m, the min-p set, is exact as well: an fp32 subtract, an fp32 divide and a comparison with c = (float)log(min_p).
  * The acceptance test is sample_ref.Acceptor's, applied to the penalised row with both of its sets intersected with
    C_m: a token is accepted iff it is in S_hi & C_m and its float64 key is within the same DELTA of the best key of
    S_lo & C_m. The maximum of the row is in every one of these sets, so none is empty and no case is skipped.
"""
from __future__ import annotations

import numpy as np

from tests import sample_ref as R

NEUTRAL = dict(temperature=0.0, top_k=0, top_p=1.0, seed=0, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0,
               frequency_penalty=0.0, penalty_from=0)


def params(**kw):
    """A full parameter block: the neutral one with kw over it (stop and max_pos are not part of the row rule)."""
    bad = set(kw) - set(NEUTRAL) - {"stop", "max_pos"}
    assert not bad, bad
    return {**NEUTRAL, **kw}


def penalised(P):
    return P["repetition_penalty"] != 1.0 or P["presence_penalty"] != 0.0 or P["frequency_penalty"] != 0.0


def counts(hist, pos, P, V):
    """n_i: occurrences of token i at positions penalty_from .. pos; entries outside [0, V) are not counted."""
    h = np.asarray(hist, np.int64)[max(int(P["penalty_from"]), 0):int(pos) + 1]
    h = h[(h >= 0) & (h < V)]
    return np.bincount(h, minlength=V)


def penalise(l, hist, pos, P):
    """l' in fp32, one rounding per operation; an element that is not in the window is returned bit for bit."""
    l = np.asarray(l, np.float32)
    out = l.copy()
    if not penalised(P):
        return out
    n = counts(hist, pos, P, l.size)
    rp, pp, fp = (np.float32(P[k]) for k in ("repetition_penalty", "presence_penalty", "frequency_penalty"))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in np.flatnonzero(n):
            v = l[i]
            a = np.float32(v / rp) if v > 0 else np.float32(v * rp)
            b = np.float32(a - pp)
            out[i] = np.float32(b - np.float32(fp * np.float32(n[i])))
    return out


def min_p_set(lp, P):
    """C_m as a boolean mask, exact (all True while min-p is off)."""
    lp = np.asarray(lp, np.float32)
    if P["min_p"] == 0.0:
        return np.ones(lp.size, bool)
    c = np.float32(np.log(np.float64(np.float32(P["min_p"]))))
    x = np.where(np.isnan(lp), np.float32(-np.inf), lp)
    m = x.max()
    with np.errstate(invalid="ignore", over="ignore"):
        q = ((lp - np.float32(m)).astype(np.float32) / np.float32(P["temperature"])).astype(np.float32)
        return q >= c  # a NaN fails


def greedy(l, hist, pos, P):
    return R.argmax_a8(penalise(l, hist, pos, P))


def draw(l, hist, pos, P, seq):
    """The rule's token, the sets and keys in float64."""
    lp = penalise(l, hist, pos, P)
    T = P["temperature"]
    if T == 0.0 or R.degenerate(lp):
        return R.argmax_a8(lp)
    c = R.nucleus(lp, R.top_k_set(lp, P["top_k"]), T, P["top_p"]) & min_p_set(lp, P)
    k = np.where(c, R.keys64(lp, T, P["seed"], seq, pos), -np.inf)
    return int(np.argmax(k))


def draw_fp32(l, hist, pos, P, seq):
    """An fp32 evaluation (sample_ref.draw_fp32's keys and masses), the stand-in for an implementation."""
    lp = penalise(l, hist, pos, P)
    T = P["temperature"]
    if T == 0.0 or R.degenerate(lp):
        return R.argmax_a8(lp)
    ck = R.top_k_set(lp, P["top_k"])
    c = ck
    if P["top_p"] < 1.0:
        idx = np.flatnonzero(ck)
        v = lp[idx]
        w = np.exp(((v - v.max()) / np.float32(T)).astype(np.float32)).astype(np.float32)
        order = np.argsort(-v, kind="stable")
        vs, ws = v[order], w[order].astype(np.float64)
        cum = np.cumsum(ws)
        last = np.r_[vs[1:] != vs[:-1], True]
        reach = last & (cum >= np.float64(np.float32(P["top_p"])) * cum[-1])
        tau = vs[np.flatnonzero(reach)[0]] if reach.any() else vs[-1]
        c = np.zeros_like(ck)
        c[idx[v >= tau]] = True
    c = c & min_p_set(lp, P)
    u = R.uniforms(P["seed"], seq, pos, lp.size).astype(np.float32)
    g = np.log(-np.log(u).astype(np.float32)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        k = (lp / np.float32(T)).astype(np.float32) - g
    return int(np.argmax(np.where(c, k, -np.inf)))


def accept(t, l, hist, pos, P, seq):
    """(ok, why) for a token t claimed as the draw of row l under block P, as sequence seq at position pos."""
    lp = penalise(l, hist, pos, P)
    t = int(t)
    if P["temperature"] == 0.0:
        want = R.argmax_a8(lp)
        return t == want, f"greedy row: token {t}, the argmax of the penalised row is {want}"
    a = R.Acceptor(lp, P["temperature"], P["top_k"], P["top_p"])
    if a.degenerate:
        return a.check(t, P["seed"], seq, pos)
    cm = min_p_set(lp, P)
    if 0 <= t < lp.size and not cm[t]:
        return False, f"token {t} (penalised logit {lp[t]}) fails min-p {P['min_p']} ({int(cm.sum())} of {lp.size} pass)"
    a.s_lo = a.s_lo & cm
    a.s_hi = a.s_hi & cm
    return a.check(t, P["seed"], seq, pos)
