"""numpy reference of the FP8 E4M3 K/V cache (include/sli.h SLI_DT_F8E4M3), written from the format alone.

decode  the 256-entry table: 1 sign, 4 exponent (bias 7) and 3 mantissa bits, subnormals m 2^-9, largest finite value
        448, no infinities, 0x7F / 0xFF NaN.
encode  the quantising rule from fp32: NaN -> 0x7F; every |v| > 448 (inf included) saturates to +-448; otherwise the
        nearest representable magnitude, found by comparing with the midpoints of adjacent codes, a value ON a midpoint
        going to the even code; the sign bit is the input's (-0 -> 0x80).
Model8  refmath.Model64 with every new K/V row rounded through encode / decode where Model64 rounds to fp16, in
        float64 (`dtype=np.float32`: the same restatement in fp32 numpy, the reference-alone check's second run).
walk    the position-by-position, layer-by-layer comparison of that model's new K/V rows with another run's rows
        (the GPU's, or the fp32 restatement's), which adopts the other run's code where the two differ by one code
        step and the unrounded value lies within a slack of the boundary between the two codes.
"""
from __future__ import annotations

import numpy as np

from tests import refmath


def _table():
    t = np.empty(256, np.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        mag = m * 2.0 ** -9 if e == 0 else 2.0 ** (e - 7) * (1 + m / 8)
        t[b] = np.nan if (b & 0x7F) == 0x7F else (-mag if b & 0x80 else mag)
    return t


TABLE64 = _table()
TABLE = TABLE64.astype(np.float32)   # exact: every value is an fp32 (and an fp16) number
MAGS = TABLE64[:0x7F]                # the 127 finite magnitudes, ascending, MAGS[c] the value of code c
MIDS = (MAGS[:-1] + MAGS[1:]) / 2    # MIDS[c]: the boundary between codes c and c + 1 (exact in float64)
MAX = 448.0


def decode(codes):
    return TABLE[np.asarray(codes, np.uint8)]


def encode(x):
    """fp32 (or float64: the restatement's unrounded values) -> uint8 codes, the rule above."""
    x = np.asarray(x)
    a = np.abs(x.astype(np.float64))
    nan = np.isnan(a)
    a = np.minimum(np.where(nan, 0.0, a), MAX)
    lo = np.searchsorted(MIDS, a, side="left")    # MIDS[lo - 1] < a <= MIDS[lo]
    on = (lo < len(MIDS)) & (MIDS[np.minimum(lo, len(MIDS) - 1)] == a)   # a tie between codes lo and lo + 1
    code = np.where(on & (lo % 2 == 1), lo + 1, lo).astype(np.uint8)
    code |= (np.signbit(x).astype(np.uint8) << 7)
    return np.where(nan, np.uint8(0x7F), code).astype(np.uint8)


def boundary(c0, c1):
    """The magnitude that separates two adjacent codes of one sign (code values with the sign bit stripped)."""
    return MIDS[np.minimum(c0, c1)]


class Model8(refmath.Model64):
    """Model64 with an FP8 cache. forward() takes `adopt(l, pos, which, unrounded, codes) -> codes`: called for every
    new K (which 0) and V (1) row with the restatement's unrounded values and its own codes, it returns the codes the
    cache keeps (the walk below compares and adopts there). rounding=False: no rounding at all (the slack measurement).
    dtype=np.float32 runs the same statements in fp32 numpy."""

    def __init__(self, cfg, weights, rounding=True, dtype=np.float64):
        super().__init__(cfg, weights)
        self.rounding, self.dt = rounding, dtype
        # the weights in the run's own type once (fp32 arrays would be widened again at every product)
        self.w = {k: (v.astype(dtype) if isinstance(v, np.ndarray) else [a.astype(dtype) for a in v])
                  for k, v in weights.items()}
        self.kc, self.vc = self.kc.astype(dtype), self.vc.astype(dtype)

    def _c(self, a):
        return a.astype(self.dt)

    def forward(self, token, pos, adopt=None):
        c, w, R = self.c, self.w, refmath
        x = self._c(w["emb"][token])
        rows = []
        for l in range(c.n_layers):
            h = self._c(R.rmsnorm(x, w["norm"][2 * l], c.eps))
            q = self._c(R.rope(self._c(w["wq"][l] @ h), pos, self.sin, self.cos, c.head_dim))
            k = self._c(R.rope(self._c(w["wk"][l] @ h), pos, self.sin, self.cos, c.head_dim))
            v = self._c(w["wv"][l] @ h)
            rows.append((k.copy(), v.copy()))
            if self.rounding:
                kq, vq = encode(k), encode(v)
                if adopt is not None:
                    kq, vq = adopt(l, pos, 0, k, kq), adopt(l, pos, 1, v, vq)
                k, v = TABLE64[kq], TABLE64[vq]
            self.kc[l, pos] = k
            self.vc[l, pos] = v
            a = self._c(R.mha(q, self.kc[l], self.vc[l], pos, c.head_dim, c.n_heads, c.n_kv_heads))
            x1 = self._c(x + w["wo"][l] @ a)
            h = self._c(R.rmsnorm(x1, w["norm"][2 * l + 1], c.eps))
            act = self._c(R.swiglu(self._c(w["up"][l] @ h), self._c(w["gate"][l] @ h)))
            x = self._c(x1 + w["down"][l] @ act)
        h = self._c(R.rmsnorm(x, w["norm"][2 * c.n_layers], c.eps))
        self.last_rows = rows
        return self._c(w["emb"] @ h)


class Walk:
    """The comparison of Model8's new rows with another run's codes. other(l, pos, which) -> that run's uint8 row.
    A differing element must differ by exactly one code step (same sign, or the two zeros) and the reference's
    unrounded magnitude must lie within `slack` of the boundary between the two codes; then the reference adopts the
    other run's code. Anything else raises AssertionError at that element."""

    def __init__(self, other, slack):
        self.other, self.slack = other, slack
        self.flips = self.compared = 0

    def __call__(self, l, pos, which, unrounded, codes):
        theirs = np.asarray(self.other(l, pos, which), np.uint8)
        assert theirs.shape == codes.shape
        self.compared += codes.size
        diff = np.nonzero(theirs != codes)[0]
        for i in diff:
            a, b = int(codes[i]), int(theirs[i])
            ma, mb = a & 0x7F, b & 0x7F
            where = f"layer {l} pos {pos} {'KV'[which]} element {i}: reference {a:#04x} ({unrounded[i]!r}) other {b:#04x}"
            if ma == 0 and mb == 0:   # +0 against -0: the unrounded value is within the slack of zero
                assert abs(float(unrounded[i])) <= self.slack, where
            else:
                assert (a & 0x80) == (b & 0x80) and abs(ma - mb) == 1 and mb != 0x7F, "not one code step: " + where
                d = abs(abs(float(unrounded[i])) - float(boundary(ma, mb)))
                assert d <= self.slack, f"{d:.3e} from the boundary, slack {self.slack:.3e}: " + where
            self.flips += 1
        return theirs.copy()


# ---------------------------------------------------------------- the model comparison
MATS = (("wq", "T_WQ"), ("wk", "T_WK"), ("wv", "T_WV"), ("wo", "T_WO"), ("up", "T_UP"), ("gate", "T_GATE"),
        ("down", "T_DOWN"))
FLIP_CAP = 0.01  # adopted flips per compared element and run: a condition, not a measurement


def ocfg(O, cfg):
    return O.Config(cfg.vocab_size, cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim,
                    cfg.intermediate_size, cfg.num_hidden_layers, cfg.max_length, cfg.rms_norm_eps, cfg.rope_theta)


def weights(O, cfg, seed, w_dtype):
    """The weights the GPU model of (preset, seed, w_dtype) computes with, as fp32 arrays, from the oracle the way
    test_oracle.py builds Model64's: fp16-rounded (W_F16), int8-dequantised (W_I8), or the fp32 weights through the
    MXFP4 rule (tests/mxfp4_ref.py quant_dequant; the norms stay fp32)."""
    oc = ocfg(O, cfg)
    om = O.Model(oc, seed=seed, wmode={"f16": O.W_F16, "i8": O.W_I8, "mxfp4": O.W_F32}[w_dtype])
    if w_dtype == "mxfp4":
        from tests import mxfp4_ref as mx
        fix = mx.quant_dequant
    else:
        fix = lambda a: a
    W = {"emb": fix(om.weight(O.T_EMB)).copy(),
         "norm": [om.weight(O.T_NORM, i).copy() for i in range(2 * oc.n_layers + 1)]}
    for k, kind in MATS:
        W[k] = [fix(om.weight(getattr(O, kind), l)).copy() for l in range(oc.n_layers)]
    om.close()
    return oc, W


def pad_prompt(prompt, n, vocab, seed):
    """A teacher-forced run: the prompt continued to n tokens with fixed pseudo-random ones (no greedy feedback)."""
    r = np.random.default_rng(1000 + seed)
    return list(prompt) + [int(t) for t in r.integers(1, vocab, n - len(prompt))]


def unrounded_rows(oc, W, tokens, dtype=np.float64):
    """The restatement without any cache rounding: per position and layer the (k, v) rows, and the logits."""
    m = Model8(oc, W, rounding=False, dtype=dtype)
    rows, logits = [], []
    for p, t in enumerate(tokens):
        logits.append(m.forward(int(t), p))
        rows.append(m.last_rows)
    return rows, np.array(logits)


def slack_from(rows64, other):
    """4 x the largest |K/V row difference| between the unrounded reference and another unrounded run
    (other(l, pos, which) -> that run's fp32 row)."""
    worst = 0.0
    for p, per_layer in enumerate(rows64):
        for l, kv in enumerate(per_layer):
            for which in (0, 1):
                worst = max(worst, float(np.abs(kv[which] - other(l, p, which)).max()))
    return 4.0 * worst


def walk_run(oc, W, tokens, other_codes, slack, start=0, cache=None):
    """The FP8 reference over `tokens` at positions start.., adopting other_codes(l, pos, which) within the slack.
    cache: (kc, vc) decoded rows [L, start, KV] the run starts from. Returns (logits, Walk)."""
    m = Model8(oc, W)
    if cache is not None:
        m.kc[:, :start], m.vc[:, :start] = cache
    w = Walk(other_codes, slack)
    logits = np.array([m.forward(int(t), start + i, adopt=w) for i, t in enumerate(tokens)])
    return logits, w


def check_logits(got, ref, what=""):
    """Every position within 1e-3 of the reference; the argmax equal wherever the reference's top-2 gap exceeds 2e-3."""
    err = float(np.abs(got - ref).max())
    print(f"{what}: max|dlogit| vs the FP8 float64 reference {err:.3e}")
    assert err <= 1e-3, (what, err)
    s = np.sort(ref, axis=-1)
    clear = (s[:, -1] - s[:, -2]) > 2e-3
    assert np.array_equal(np.argmax(got, -1)[clear], np.argmax(ref, -1)[clear]), what


def check_flips(w, what="", cap=FLIP_CAP):
    print(f"{what}: {w.flips} adopted code flips of {w.compared} compared elements, slack {w.slack:.3e}")
    assert w.flips <= cap * w.compared, (what, w.flips, w.compared)
