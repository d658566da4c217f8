"""numpy restatement of the sampling rule of include/sli.h (sli_sample), and the acceptance test the GPU checks use.

The rule is restated from the header's text, not from the kernel: the hash vectorised, C_k exact, the nucleus and the
Gumbel keys in float64. The acceptance test is derived, not tuned:

  * Sets. C_k is exact. S_lo = the nucleus at top_p - EPS and S_hi = the nucleus at min(1, top_p + EPS), both in
    float64, EPS = 1e-4: an fp32 exp of an argument of magnitude <= 88 is within 88 * 2^-23 ~ 1e-5 relative, and
    1e-4 leaves 10x. S_lo is a subset of S_hi.
  * A token t is accepted iff t is in S_hi and key64[t] >= max(key64[S_lo]) - DELTA with
    DELTA = 8 * 2^-23 * max(1, max |key64|) over the finite keys of S_hi: a correctly rounded fp32 evaluation of the
    keys measured at most 0.12 DELTA away from float64 (160 draws, V = 128 256, T from 0.05 to 2).
  * A row without a finite maximum: exactly the first-maximum index that sli_argmax returns.
"""
from __future__ import annotations

import numpy as np

SAMPLE_STREAM = 12  # SLI_SAMPLE_STREAM
EPS = 1e-4
M32 = np.uint64(0xFFFFFFFF)


def _hash32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def rng_u32(seed, stream, idx):
    """sli_synth.h sli_rng_u32, vectorised over idx (uint64 arithmetic masked to 32 bits)."""
    idx = np.asarray(idx, np.uint64)
    seed, stream = np.uint64(seed & 0xFFFFFFFF), np.uint64(stream & 0xFFFFFFFF)
    h = _hash32(((seed * np.uint64(0x9E3779B9)) & M32) ^ _hash32((stream + np.uint64(0x632BE5AB)) & M32))
    h = _hash32(h ^ (idx & M32))
    return _hash32(h ^ (idx >> np.uint64(32)) ^ np.uint64(0x85EBCA6B))


def uniforms(seed, seq, pos, V):
    """u_i = (2 (h_i >> 9) + 1) 2^-24 for i < V, as float64 (every value is exact in fp32)."""
    stream = (SAMPLE_STREAM << 16) | (seq & 0xFFFF)
    idx = (np.uint64(pos & 0xFFFFFFFF) << np.uint64(32)) | np.arange(V, dtype=np.uint64)
    h = rng_u32(seed, stream, idx)
    return (2.0 * (h >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def argmax_a8(l):
    """sli_argmax: std::max_element's scan `if (*best < *it) best = it` (first maximum; a NaN never displaces and, at
    index 0, is never displaced)."""
    l = np.asarray(l, np.float32)
    if np.isnan(l[0]):
        return 0
    x = np.where(np.isnan(l), -np.inf, l.astype(np.float64))
    return int(np.argmax(x))  # first index of the maximum; -0 == +0


def degenerate(l):
    """No finite maximum: every logit NaN or -inf, or a +inf present."""
    l = np.asarray(l, np.float32)
    return bool(np.any(l == np.inf)) or not bool(np.any(np.isfinite(l)))


def top_k_set(l, top_k):
    """C_k as a boolean mask, exact: the finite logits >= the k-th largest (NaN counted as -inf)."""
    l = np.asarray(l, np.float32)
    cand = np.isfinite(l)
    V = l.size
    if top_k <= 0 or top_k >= V:
        return cand
    x = np.where(np.isnan(l), np.float32(-np.inf), l)
    tau = np.partition(x, V - top_k)[V - top_k]  # the k-th largest with multiplicity
    return cand & (x >= tau)  # fp32 comparison: -0 == +0


def nucleus(l, ck, T, top_p):
    """C within C_k in float64: the logits >= the largest value v whose upper mass reaches top_p."""
    if top_p >= 1.0:
        return ck.copy()
    l64 = np.asarray(l, np.float32).astype(np.float64)
    idx = np.flatnonzero(ck)
    v = l64[idx]
    w = np.exp((v - v.max()) / T)
    order = np.argsort(-v, kind="stable")
    vs, ws = v[order], w[order]
    cum = np.cumsum(ws) / ws.sum()
    # the upper mass of value v includes all its ties: the cumulative sum at the LAST element of each run of equals
    last = np.r_[vs[1:] != vs[:-1], True]
    reach = last & (cum >= top_p)
    tau = vs[np.flatnonzero(reach)[0]] if reach.any() else vs[-1]
    out = np.zeros_like(ck)
    out[idx[v >= tau]] = True
    return out


def keys64(l, T, seed, seq, pos):
    l64 = np.asarray(l, np.float32).astype(np.float64)
    u = uniforms(seed, seq, pos, l64.size)
    with np.errstate(invalid="ignore", over="ignore"):
        return l64 / T - np.log(-np.log(u))


def draw(l, T, top_k, top_p, seed, seq, pos):
    """The rule's token in float64."""
    if degenerate(l):
        return argmax_a8(l)
    c = nucleus(l, top_k_set(l, top_k), T, top_p)
    k = np.where(c, keys64(l, T, seed, seq, pos), -np.inf)
    return int(np.argmax(k))


def draw_fp32(l, T, top_k, top_p, seed, seq, pos):
    """An fp32 evaluation of the rule (keys and masses in float32), the stand-in for an implementation."""
    if degenerate(l):
        return argmax_a8(l)
    l = np.asarray(l, np.float32)
    ck = top_k_set(l, top_k)
    c = ck
    if top_p < 1.0:
        idx = np.flatnonzero(ck)
        v = l[idx]
        w = np.exp(((v - v.max()) / np.float32(T)).astype(np.float32)).astype(np.float32)
        order = np.argsort(-v, kind="stable")
        vs, ws = v[order], w[order].astype(np.float64)
        cum = np.cumsum(ws)
        last = np.r_[vs[1:] != vs[:-1], True]
        reach = last & (cum >= np.float64(np.float32(top_p)) * cum[-1])
        tau = vs[np.flatnonzero(reach)[0]] if reach.any() else vs[-1]
        c = np.zeros_like(ck)
        c[idx[v >= tau]] = True
    u = uniforms(seed, seq, pos, l.size).astype(np.float32)
    g = np.log(-np.log(u).astype(np.float32)).astype(np.float32)
    with np.errstate(over="ignore"):
        k = (l / np.float32(T)).astype(np.float32) - g
    return int(np.argmax(np.where(c, k, -np.inf)))


def chi2_sf(x, dof):
    """P(chi-square with dof degrees of freedom > x) = Q(dof / 2, x / 2), the regularised upper incomplete gamma:
    its series below a + 1, Lentz's continued fraction above (float64 throughout)."""
    import math
    a, x = dof / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1:
        term = total = 1.0 / a
        n = a
        while abs(term) > abs(total) * 1e-17:
            n += 1
            term *= x / n
            total += term
        return 1.0 - lead * total
    tiny = 1e-300
    b = x + 1 - a
    c, d = 1 / tiny, 1 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        h *= d * c
        if abs(d * c - 1) < 1e-16:
            break
    return lead * h


def chi2_quantile(tail, dof):
    """x with chi2_sf(x, dof) = tail, by bisection."""
    lo, hi = 0.0, dof + 100.0 * (dof ** 0.5 + 10)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi2_sf(mid, dof) > tail else (lo, mid)
    return hi


class Acceptor:
    """The acceptance test for draws from one row l under one (T, top_k, top_p): the sets are computed once, the keys
    per draw. check(t, seed, seq, pos) -> (ok, why)."""

    def __init__(self, l, T, top_k, top_p):
        self.l = np.asarray(l, np.float32)
        self.T = T
        self.degenerate = degenerate(self.l)
        if self.degenerate:
            self.want = argmax_a8(self.l)
            return
        self.ck = top_k_set(self.l, top_k)
        self.s_lo = nucleus(self.l, self.ck, T, top_p - EPS if top_p - EPS > 0 else 1e-300)
        self.s_hi = nucleus(self.l, self.ck, T, min(1.0, top_p + EPS))

    def check(self, t, seed, seq, pos):
        l, t = self.l, int(t)
        if not 0 <= t < l.size:
            return False, f"token {t} outside [0, {l.size})"
        if self.degenerate:
            return t == self.want, f"degenerate row: token {t}, sli_argmax gives {self.want}"
        if not self.s_hi[t]:
            return False, f"token {t} (logit {l[t]}) outside the candidate set ({int(self.s_hi.sum())} of {l.size})"
        k = keys64(l, self.T, seed, seq, pos)
        delta = 8 * 2.0 ** -23 * max(1.0, float(np.abs(k[self.s_hi]).max()))
        best = k[self.s_lo].max()
        return bool(k[t] >= best - delta), f"token {t} key {k[t]!r} below the best {best!r} by more than {delta!r}"


def accept(t, l, T, top_k, top_p, seed, seq, pos):
    """(ok, why) for a token t claimed as the draw of row l."""
    return Acceptor(l, T, top_k, top_p).check(t, seed, seq, pos)
