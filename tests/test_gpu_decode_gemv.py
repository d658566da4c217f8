"""The batch-1 decode GEMVs (simplellminference_amd/csrc/gemv.h) one launch at a time, through the kernel-level entry of
sli.h ("decode stages, for tests and labs"), against the float64 reference tests/gemv_ref.py (itself held to the C
oracle by test_gemv_ref_cpu.py). The entry launches the engine's own code objects on the engine's own plans, made as if
the chip had `cus` compute units: gemv_ref.CELLS are matrices of a few hundred rows whose plans have the schedule
class of every launch of a production model (test_decode_stage_cpu.py holds that cover, per weight type).

Every output is filled with NaN sentinels before the launch; the q/k/v cache is three layers' worth of memory with the
middle layer under test; every launch runs twice.

Bars (derivations in gemv_ref.py, bgemm_ref.py and prefill_ref.py next to each bound):
  (a) exact inputs (integer weights, power-of-two row / block scales; x integers; with a norm eps = 0, power-of-two
      norm weights and x a signed shuffle of 11 K / 16 ones and 5 K / 16 sevens, so inv = 0.25 in every summation
      order, asserted; sum of absolute terms below 2^24 grid units, asserted): store, K-part and logits rows, the
      in-place residual and the K-split residual equal the reference BIT FOR BIT; q / k / v at position 0 too, the
      fp16 and FP8 cache values being the exact roundings; position > 0 within prefill_ref.rope_tol, SwiGLU within
      gemv_ref.swiglu_tol. Merged input: all live m_s equal, l_s = 1, 1, 2, 4, ..., integer o_s, dead splits and pad
      words NaN: exact for every ns.
  (b) realistic inputs (normal x, W / sqrt(K), eps 1e-5, distinct m_s): sums within 4 eps32 sqrt(K) (|W| @ |h|) of the
      float64 sum of the same rounded operands, plus |W| @ dh for the staged input's own bound (norm: NORM_RTOL and two
      roundings; merge: the expf and fma chain), each passed through the epilogue's derivative.
  (c) keys: the maximum over keys[0 .. grid) names the value and the lowest index of the maximum of the kernel's own
      logits row: a planted tie across workgroups, -0 against +0, an odd nrows, vocab_off > 0.
  (d) nothing else is written: every cache element but (head, pos) of the middle layer, y / logits / act / part beyond
      their rows, keys beyond the grid; the inputs are unchanged.
  (e) each launch twice, bit-identical; cus = the device's count == cus 0, bit for bit.
  (f) FP8 codes: bgemm_ref.f8_check under kv8_ref.FLIP_CAP; none is needed at position 0 of the exact family.

Measured on an MI355X (24 tests, 4.5 s): every cell of (a) is bit-exact; no FP8 code needed its neighbour (0 of 3,584
per weight type); (b) holds as stated, the largest error / bound per role (over the four weight types): q 0.016,
gate/up < 0.001, wo plain 0.027, down 0.001, wo merged 0.004, K-part 0.003, logits 0.007. The bounds are worst-case in
sqrt(K) and carry NORM_RTOL = 2e-6 (17 eps32) on the norm factor, so a correct kernel sits far inside them: what bites
on arithmetic is (a), and (b) guards the realistic ranges (an overflowing expf, an unscaled norm). Nothing was found
wrong in gemv.h.

What the first run found in the test's own bounds, both fixed in gemv_ref.swiglu_tol with the reasoning beside it:
bgemm_ref.swiglu_tol cancels its 4 eps32 |act| term against the split terms it subtracts where |act| << 2^-24, and
act_tol has no underflow term, while the exact family's integer sums reach g < -87.3, where the fp32 sigmoid lies below
the smallest normal number (9 gate/up cells of the fp32 weight type at errors of 1e-25 .. 1e-34 against a bound of 0).

That it bites (scratch builds of gemv.h with one arithmetic-only change each, not committed; this file run once per
build; tests failing of 24, and the bar that caught it first):
  1 norm factor not applied (XStage)          16  (a) q / k / v, act, logits of every weight type unequal; keys; (e)
  2 row scale after the rotation               1  (a) int8 q / k at position > 0 outside rope_tol (the only row scales)
  3 sin / cos of position 0                    4  (a) q / k at positions 17 and T - 1 outside rope_tol, every weight type
  4 EpiStoreSum adds the parts last to first   4  (a) down np 2 / 4 residual off by 1 / 3 on the planted rows. The
                                                 first run missed it (0): integer parts add exactly in any order, and
                                                 (b) allows an ulp; gemv_ref.plant_order* now make the order show
  5 a dead split consumed (ns + 1)             4  (a) merged wo and K-part NaN from the NaN of the dead split
  6 M taken from split 0                       4  (b) merged wo inf / NaN: expf overflows where split 0 lies 120 below
                                                 the maximum. The first run missed it (0): the merge is shift-invariant,
                                                 so with m_s a few units apart it is the same function to rounding;
                                                 real_merge_parts now puts split 0 far below on every other head
  7 argmax key before the row scale            1  (c) int8 keys name another row than the logits' maximum
  8 the last column part dropped              15  (a) every column-split cell (q/k/v, gate/up, logits, fp32 / MXFP4
                                                 wo); the fp16 / int8 wo cell with csplit 4 had only the part wholly
                                                 past the row end to lose, so (WO, 4096, cus 2, 12 rows) was added
(Rows 1, 2, 3, 5, 7 and 8 were counted before the changes made for rows 4, 6 and 8, which only add checks.)
"""
import zlib

import numpy as np
import pytest

from tests import bgemm_ref as B
from tests import gemv_ref as G
from tests import kv8_ref as F8
from tests import prefill_ref as P
from tests.test_gpu_prefill_kernels import _hold, _is_sentinel, _sentinel

pytestmark = pytest.mark.gpu

SENT8 = 0x7F
SENT64 = 0x7FC5A5A57FC5A5A5
PAD = 5  # sentinel elements behind every output
RATIOS = {}


def _seed(cell, wt, fam):
    return zlib.crc32(f"{G.cell_id(cell)}|{wt}|{fam}".encode()) & 0x7FFFFFFF


def _t(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wdev(torch, W, wt):
    """(w, scales) device tensors of gemv_ref's weights."""
    if wt == "mxfp4":
        return _t(torch, W[0]), _t(torch, W[1])
    return _t(torch, W), None


def _weights(N, K, wt, fam, seed):
    """(W, row scales, float64 values, grid step or None)."""
    if fam == "exact":
        return G.exact_weights(N, K, wt, seed)
    return G.real_weights(N, K, wt, seed) + (None,)


def _ratio(role, got, ref, tol):
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, 0.0)
    RATIOS[role] = max(RATIOS.get(role, 0.0), float(np.nanmax(r)) if r.size else 0.0)


def _tail_ok(fails, tag, arr, n, what):
    """arr[n:] is still the sentinel and arr[:n] is all written."""
    sent = (arr == np.uint64(SENT64)) if arr.dtype == np.uint64 else _is_sentinel(arr)
    if not sent[n:].all():
        fails.append(f"{tag}: {what} written past element {n}")
    if sent[:n].any():
        fails.append(f"{tag}: {int(sent[:n].sum())} elements of {what} not written")


def _same(fails, tag, a, b, what):
    if not np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)):
        fails.append(f"{tag}: {what}")


def _unchanged(fails, tag, pairs):
    for name, dev, host in pairs:
        if dev is not None and not np.array_equal(dev.cpu().numpy().view(np.uint8), np.ascontiguousarray(host).view(np.uint8)):
            fails.append(f"{tag}: the input {name} was changed")


def _twice(fails, tag, run):
    a, b = run(), run()
    for k in a:
        if k != "plan":
            _same(fails, tag, a[k], b[k], f"{k} differs between two launches")
    return a


def _norm_input(K, fam, seed, np_):
    """x, norm_w, eps, parts, the float64 staged input h and its bound dh (exact family: 0), the grid step of h."""
    r = np.random.default_rng(seed)
    if fam == "exact":
        x1, nw, eps = G.exact_x_norm(K, seed), G.exact_norm_w(K, seed), 0.0
        parts = G.exact_parts(np_, K, seed) if np_ else None
        x = x1 if parts is None else (x1 - parts.sum(axis=0)).astype(np.float32)
        if parts is not None:
            x, parts = G.plant_order(x, parts, x1)  # XStageSum's order of the adds shows
        assert np.array_equal(G.x1_sum(x, parts), x1)
        h = x1.astype(np.float64) * 0.25 * nw
        return x, nw, eps, parts, h, np.zeros(K), 0.25
    x = r.standard_normal(K).astype(np.float32)
    nw = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    parts = (0.5 * r.standard_normal((np_, K))).astype(np.float32) if np_ else None
    h, _ = G.staged_norm(G.x1_sum(x, parts), nw, G.EPS)
    return x, nw, G.EPS, parts, h, G.staged_norm_tol(h), None


def _sums(Wv, h, dh, K, unit, h_unit):
    """Y, dY of the launch's row sums."""
    Y, A = G.sums(Wv, h)
    if unit is not None:
        assert G.exact_units(Wv, h, unit * h_unit) < 2 ** 24  # the condition of every bit-exact claim
        return Y, np.zeros_like(Y)
    return Y, G.sum_tol(A, K) + np.abs(Wv) @ dh


def _cells(role, wt, pred=lambda s: True):
    return [c for c in G.CELLS if c[0] == role and G.cell_takes(c, wt) and pred(c[3])]


def _finish(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:25])


# ---------------------------------------------------------------- q/k/v
@pytest.fixture(scope="module")
def tables(gpu):
    from simplellminference_amd import ops
    out = {}
    for hd in (64, 128):
        s, c = ops.rope_cache(hd, G.T, 10000.0)
        out[hd] = (s, c, s.cpu().numpy(), c.cpu().numpy())
        assert (out[hd][2][0] == 0).all() and (out[hd][3][0] == 1).all()  # position 0: the identity, exactly
    return out


def _cache(torch, kv, shape):
    if kv == "f8":
        return torch.full(shape, SENT8, dtype=torch.uint8, device="cuda")
    return _sentinel(torch, shape, kv == "f16")


def _check_cache(fails, tag, got, ref, tol, kv, pos, flips):
    """One layer's cache rows [3][hkv][T][hd]: row pos of the middle layer against ref [hkv][hd], the rest untouched."""
    written = np.zeros(got.shape, bool)
    written[1, :, pos, :] = True
    sent = (got == SENT8) if kv == "f8" else _is_sentinel(got)
    if (~sent & ~written).any():
        fails.append(f"{tag}: cache written outside (head, pos), first at {np.argwhere(~sent & ~written)[0].tolist()}")
    row = got[1, :, pos, :]
    if kv == "f8":
        ok, flip = B.f8_check(row, ref, tol)
        if not ok.all():
            fails.append(f"{tag}: {int((~ok).sum())} FP8 codes outside the accepted pair")
        flips[0] += int(flip.sum())
        flips[1] += flip.size
        if not np.any(tol > 0) and flip.any():
            fails.append(f"{tag}: an exact value took the neighbouring FP8 code")
    elif kv == "f16":
        if sent[1, :, pos, :].any():
            fails.append(f"{tag}: cache row not written")
        ok = P.within_f16_rounding(row, ref, tol)
        if not ok.all():
            fails.append(f"{tag}: {int((~ok).sum())} fp16 cache values are not roundings of the reference")
    else:
        _hold(fails, tag, row, ref, tol)


@pytest.mark.parametrize("wt", G.WTS)
def test_qkv(gpu, tables, wt):
    from simplellminference_amd import ops
    torch, fails, flips = gpu, [], [0, 0]
    kvs = ("f32", "f16") if wt == "f32" else ("f32", "f16", "f8")
    for i, cell in enumerate(_cells(G.QKV, wt)):
        _, K, cus, s = cell
        hq, hkv, hd = s["hq"], s["hkv"], s["hd"]
        N, nq, nk = (hq + 2 * hkv) * hd, hq * hd, hkv * hd
        sin_d, cos_d, sin_t, cos_t = tables[hd]
        for fam in ("exact", "real"):
            seed = _seed(cell, wt, fam)
            W, rs, Wv, unit = _weights(N, K, wt, fam, seed)
            x, nw, eps, _, h, dh, hu = _norm_input(K, fam, seed, 0)
            Y, dY = _sums(Wv, h, dh, K, unit, hu)
            a, da = G.scaled(Y, dY, rs)
            wd, sd = _wdev(torch, W, wt)
            xd, nwd, rsd = _t(torch, x), _t(torch, nw), _t(torch, rs)
            for j, kv in enumerate(kvs):
                pos = (0, 17, G.T - 1)[(i + j) % 3] if fam == "exact" else (17, G.T - 1, 5)[(i + j) % 3]
                tag = f"{G.cell_id(cell)} {wt} {fam} kv {kv} pos {pos}"
                pd = torch.tensor([pos], dtype=torch.int32, device="cuda")

                def run():
                    q = _sentinel(torch, (nq + PAD,), False)
                    kc, vc = _cache(torch, kv, (3, hkv, G.T, hd)), _cache(torch, kv, (3, hkv, G.T, hd))
                    p = ops.decode_gemv_qkv(xd, nwd, eps, wd, q[:nq], kc[1], vc[1], pd, sin_d, cos_d, hq, hkv, hd,
                                            row_scale=rsd, scales=sd, kv_dtype="f8" if kv == "f8" else None, cus=cus)
                    return dict(q=q.cpu().numpy(), k=kc.cpu().numpy(), v=vc.cpu().numpy(), plan=p)
                out = _twice(fails, tag, run)
                ps = np.array([pos])
                qr = P.rope_rows(a[None, :nq], ps, sin_t, cos_t, hd)[0]
                kr = P.rope_rows(a[None, nq:nq + nk], ps, sin_t, cos_t, hd)[0].reshape(hkv, hd)
                vr = a[nq + nk:].reshape(hkv, hd)
                if pos == 0 and fam == "exact":
                    qt, kt = np.zeros(nq), np.zeros((hkv, hd))
                else:
                    qt = P.rope_tol(a[None, :nq], ps, sin_t, cos_t, hd, da[None, :nq])[0]
                    kt = P.rope_tol(a[None, nq:nq + nk], ps, sin_t, cos_t, hd, da[None, nq:nq + nk])[0].reshape(hkv, hd)
                vt = da[nq + nk:].reshape(hkv, hd)
                _tail_ok(fails, tag, out["q"], nq, "q")
                _hold(fails, tag + " q", out["q"][:nq], qr, qt)
                _check_cache(fails, tag + " k", out["k"], kr, kt, kv, pos, flips)
                _check_cache(fails, tag + " v", out["v"], vr, vt, kv, pos, flips)
                if fam == "real":
                    _ratio("qkv", out["q"][:nq], qr, qt)
            _unchanged(fails, G.cell_id(cell), (("x", xd, x), ("norm_w", nwd, nw), ("W", wd, W[0] if wt == "mxfp4" else W)))
    print(f"qkv {wt}: {flips[0]} FP8 neighbour codes of {flips[1]}; largest err / bound {RATIOS.get('qkv', 0):.3f}")
    assert flips[0] <= F8.FLIP_CAP * max(flips[1], 1), flips
    _finish(fails)


# ---------------------------------------------------------------- gate/up
@pytest.mark.parametrize("wt", G.WTS)
def test_gate_up(gpu, wt):
    from simplellminference_amd import ops
    torch, fails = gpu, []
    for i, cell in enumerate(_cells(G.GATE_UP, wt)):
        _, K, cus, s = cell
        inter, np_ = s["inter"], s.get("np", 0)
        for fam in ("exact", "real"):
            seed = _seed(cell, wt, fam)
            silu = (i + (fam == "real")) % 2
            tag = f"{G.cell_id(cell)} {wt} {fam} silu {silu}"
            W, rs, Wv, unit = _weights(2 * inter, K, wt, fam, seed)
            x, nw, eps, parts, h, dh, hu = _norm_input(K, fam, seed, np_)
            Y, dY = _sums(Wv, h, dh, K, unit, hu)
            a, da = G.scaled(Y, dY, rs)
            wd, sd = _wdev(torch, W, wt)
            xd, nwd, rsd, pd = _t(torch, x), _t(torch, nw), _t(torch, rs), _t(torch, parts)

            def run():
                act = _sentinel(torch, (inter + PAD,), False)
                p = ops.decode_gemv_gate_up(xd, nwd, eps, wd, act, act_mode=silu, parts=pd, row_scale=rsd, scales=sd, cus=cus)
                return dict(act=act.cpu().numpy(), plan=p)
            out = _twice(fails, tag, run)
            g, u = a[:inter], a[inter:]
            with np.errstate(over="ignore"):
                ref, tol = P.act(g, u, silu), G.swiglu_tol(g, u, silu, da[:inter], da[inter:])
            _tail_ok(fails, tag, out["act"], inter, "act")
            _hold(fails, tag, out["act"][:inter], ref, tol)
            if fam == "real":
                _ratio("gate_up", out["act"][:inter], ref, tol)
            _unchanged(fails, tag, (("x", xd, x), ("norm_w", nwd, nw), ("parts", pd, parts)))
    print(f"gate_up {wt}: largest err / bound {RATIOS.get('gate_up', 0):.3f}")
    _finish(fails)


# ---------------------------------------------------------------- wo and down (store epilogues)
def _run_store(torch, fn, nrows, resid, mode):
    """mode "none" / "separate" / "inplace": the residual of a store launch. fn(y, resid tensor) launches."""
    y = _sentinel(torch, (nrows + PAD,), False)
    r = None
    if mode == "inplace":
        y[:nrows] = _t(torch, resid)
        r = y
    elif mode == "separate":
        r = _t(torch, resid)
    p = fn(y, r)
    return dict(y=y.cpu().numpy(), plan=p)


def _check_store(fails, tag, role, out, nrows, a, da, resid, exact):
    y = a if resid is None else resid.astype(np.float64) + a
    tol = np.zeros(nrows) if exact else da + G.U32 * np.abs(y)
    _tail_ok(fails, tag, out["y"], nrows, "y")
    _hold(fails, tag, out["y"][:nrows], y, tol)
    if not exact:
        _ratio(role, out["y"][:nrows], y, tol)


def _plain_x(K, fam, seed):
    r = np.random.default_rng(seed + 5)
    return (r.integers(-4, 5, K) if fam == "exact" else r.standard_normal(K)).astype(np.float32)


def _resid(n, fam, seed):
    r = np.random.default_rng(seed + 6)
    return (r.integers(-8, 9, n) if fam == "exact" else r.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("wt", G.WTS)
def test_wo_plain_and_down(gpu, wt):
    from simplellminference_amd import ops
    torch, fails = gpu, []
    cells = _cells(G.WO, wt, lambda s: "hq" not in s) + _cells(G.DOWN, wt)
    for i, cell in enumerate(cells):
        role, K, cus, s = cell
        nrows, np_ = s["nrows"], s.get("np", 0)
        name = G.ROLE_NAMES[role]
        for fam in ("exact", "real"):
            seed = _seed(cell, wt, fam)
            mode = "inplace" if np_ else ("none", "inplace", "separate")[(i + (fam == "real")) % 3]
            tag = f"{G.cell_id(cell)} {wt} {fam} resid {mode}"
            W, rs, Wv, unit = _weights(nrows, K, wt, fam, seed)
            x = _plain_x(K, fam, seed)
            Y, dY = _sums(Wv, x.astype(np.float64), np.zeros(K), K, unit, 1.0)
            a, da = G.scaled(Y, dY, rs)
            resid = None if mode == "none" else _resid(nrows, fam, seed)
            parts = None
            if np_:
                parts = G.exact_parts(np_, nrows, seed) if fam == "exact" else \
                    np.random.default_rng(seed + 2).standard_normal((np_, nrows)).astype(np.float32)
            if np_ and fam == "exact":
                resid, parts = G.plant_order_resid(resid, parts)  # EpiStoreSum's order of the adds shows
            x1 = resid if parts is None else G.x1_sum(resid, parts)  # the K-split residual, bit for bit
            wd, sd = _wdev(torch, W, wt)
            xd, rsd, pd = _t(torch, x), _t(torch, rs), _t(torch, parts)
            if role == G.WO:
                fn = lambda y, r: ops.decode_gemv_wo(wd, y=y, x=xd, resid=r, row_scale=rsd, scales=sd, cus=cus)
            else:
                fn = lambda y, r: ops.decode_gemv_down(xd, wd, y, resid=r, parts=pd, row_scale=rsd, scales=sd, cus=cus)
            out = _twice(fails, tag, lambda: _run_store(torch, fn, nrows, resid, mode))
            _check_store(fails, tag, name, out, nrows, a, da, x1, fam == "exact")
            _unchanged(fails, tag, (("x", xd, x), ("parts", pd, parts), ("W", wd, W[0] if wt == "mxfp4" else W)))
    print(f"wo / down {wt}: largest err / bound {RATIOS.get('wo', 0):.3f} / {RATIOS.get('down', 0):.3f}")
    _finish(fails)


@pytest.mark.parametrize("wt", G.WTS)
def test_wo_merged(gpu, wt):
    """The merge-staged wo (XStageMerge, NS 8 and 16) and the K-split wo (EpiKPart) at every position class."""
    from simplellminference_amd import ops
    torch, fails = gpu, []
    for i, cell in enumerate(_cells(G.WO, wt, lambda s: "hq" in s)):
        _, K, cus, s = cell
        nrows, heads, hd, ms, ks = s["nrows"], s["hq"], s["hd"], s["max_splits"], s.get("ks", 1)
        for fam in ("exact", "real"):
            seed = _seed(cell, wt, fam)
            W, rs, Wv, unit = _weights(nrows, K, wt, fam, seed)
            wd, sd = _wdev(torch, W, wt)
            rsd = _t(torch, rs)
            for pos in G.merge_positions(ms):
                ns = G.live_splits(pos, G.PPWG, ms)
                tag = f"{G.cell_id(cell)} {wt} {fam} pos {pos} ns {ns}"
                part = (G.exact_merge_parts if fam == "exact" else G.real_merge_parts)(heads, ms, hd, ns, seed + pos)
                h, dh = G.merge(part, ns, hd)
                if fam == "exact":
                    assert B.is_f32(h)
                    dh = np.zeros(K)
                hu = 2.0 ** -(ns - 1)
                partd = _t(torch, part)
                pd = torch.tensor([pos], dtype=torch.int32, device="cuda")
                if ks == 1:
                    Y, dY = _sums(Wv, h, dh, K, unit, hu)
                    a, da = G.scaled(Y, dY, rs)
                    mode = ("inplace", "none", "separate")[(i + pos) % 3]
                    resid = None if mode == "none" else _resid(nrows, fam, seed)
                    fn = lambda y, r: ops.decode_gemv_wo(wd, y=y, resid=r, part=partd, pos=pd, ppwg=G.PPWG, hd=hd,
                                                         row_scale=rsd, scales=sd, cus=cus)
                    out = _twice(fails, tag, lambda: _run_store(torch, fn, nrows, resid, mode))
                    _check_store(fails, tag, "wo_merged", out, nrows, a, da, resid, fam == "exact")
                else:
                    Wk, kc = G.kpart_view(Wv, ks), K // ks
                    ref, tol = np.empty((ks, nrows)), np.empty((ks, nrows))
                    for k in range(ks):
                        Y, dY = _sums(Wk[k], h[k * kc:(k + 1) * kc], dh[k * kc:(k + 1) * kc], kc, unit, hu)
                        ref[k], tol[k] = G.scaled(Y, dY, rs)

                    def run():
                        kp = _sentinel(torch, (ks * nrows + PAD,), False)
                        p = ops.decode_gemv_wo(wd, part=partd, pos=pd, ppwg=G.PPWG, hd=hd, ks=ks,
                                               kpart=kp[:ks * nrows].view(ks, nrows), row_scale=rsd, scales=sd, cus=cus)
                        return dict(kpart=kp.cpu().numpy(), plan=p)
                    out = _twice(fails, tag, run)
                    _tail_ok(fails, tag, out["kpart"], ks * nrows, "kpart")
                    _hold(fails, tag, out["kpart"][:ks * nrows].reshape(ks, nrows), ref, tol)
                    if fam == "real":
                        _ratio("wo_kpart", out["kpart"][:ks * nrows].reshape(ks, nrows), ref, tol)
                _unchanged(fails, tag, (("part", partd, part),))
    print(f"wo merged / K-split {wt}: largest err / bound {RATIOS.get('wo_merged', 0):.3f} / {RATIOS.get('wo_kpart', 0):.3f}")
    _finish(fails)


# ---------------------------------------------------------------- logits and keys
def _run_logits(torch, ops, xd, nwd, eps, wd, sd, rsd, nrows, cus, voff):
    logits = _sentinel(torch, (nrows + PAD,), False)
    keys = torch.full(((cus or 512) + 3,), SENT64, dtype=torch.int64, device="cuda")
    p = ops.decode_gemv_logits(xd, nwd, eps, wd, logits, keys, vocab_off=voff, row_scale=rsd, scales=sd, cus=cus)
    return dict(logits=logits.cpu().numpy(), keys=keys.cpu().numpy().view(np.uint64), plan=p)


def _check_keys(fails, tag, out, nrows, voff):
    grid = out["plan"]["grid"]
    _tail_ok(fails, tag, out["keys"], grid, "keys")
    want = B.best_key(out["logits"][:nrows], voff)
    got = int(out["keys"][:grid].max())
    if got != want:
        fails.append(f"{tag}: key names {B.key_parts(got)}, the logits row's maximum is {B.key_parts(want)}")


@pytest.mark.parametrize("wt", G.WTS)
def test_logits(gpu, wt):
    from simplellminference_amd import ops
    torch, fails = gpu, []
    for i, cell in enumerate(_cells(G.LOGITS, wt)):
        _, K, cus, s = cell
        nrows = s["nrows"]
        for fam in ("exact", "real"):
            seed = _seed(cell, wt, fam)
            voff = (G.VOCAB_OFF, 0)[(i + (fam == "real")) % 2]
            tag = f"{G.cell_id(cell)} {wt} {fam} vocab_off {voff}"
            W, rs, Wv, unit = _weights(nrows, K, wt, fam, seed)
            x, nw, eps, _, h, dh, hu = _norm_input(K, fam, seed, 0)
            Y, dY = _sums(Wv, h, dh, K, unit, hu)
            a, da = G.scaled(Y, dY, rs)
            wd, sd = _wdev(torch, W, wt)
            xd, nwd, rsd = _t(torch, x), _t(torch, nw), _t(torch, rs)
            out = _twice(fails, tag, lambda: _run_logits(torch, ops, xd, nwd, eps, wd, sd, rsd, nrows, cus, voff))
            _tail_ok(fails, tag, out["logits"], nrows, "logits")
            _hold(fails, tag, out["logits"][:nrows], a, da)
            _check_keys(fails, tag, out, nrows, voff)
            if fam == "real":
                _ratio("logits", out["logits"][:nrows], a, da)
    print(f"logits {wt}: largest err / bound {RATIOS.get('logits', 0):.3f}")
    _finish(fails)


@pytest.mark.parametrize("wt", ("f32", "f16", "i8"))
def test_keys_ties_and_zeros(gpu, wt):
    """(c): a tie planted in the first and the last workgroup's rows (the lowest index wins), and a row of -0 below a
    row of +0 with every other logit negative (-0 counts as +0: the lower index wins). Odd nrows, vocab_off > 0."""
    from simplellminference_amd import ops
    torch, fails = gpu, []
    K, nrows, cus = 256, 61, 3
    x, nw = G.exact_x_norm(K, 11), G.exact_norm_w(K, 11)
    h = x.astype(np.float64) * 0.25 * nw
    dt = {"f32": np.float32, "f16": np.float16, "i8": np.int8}[wt]
    r = np.random.default_rng(12)
    xd, nwd = _t(torch, x), _t(torch, nw)
    # the tie: rows 2 and nrows - 1 are sign(h) * 4, the largest sum there is
    k = r.integers(-3, 4, (nrows, K))
    k[2] = k[nrows - 1] = 4 * np.sign(h)
    W = k.astype(dt)
    out = _run_logits(torch, ops, xd, nwd, 0.0, _t(torch, W), None, None, nrows, cus, G.VOCAB_OFF)
    _hold(fails, "tie", out["logits"][:nrows], k.astype(np.float64) @ h, np.zeros(nrows))
    assert out["plan"]["grid"] > 1 and out["logits"][2] == out["logits"][nrows - 1] == out["logits"][:nrows].max()
    _check_keys(fails, "tie", out, nrows, G.VOCAB_OFF)
    if B.key_parts(int(out["keys"][:out["plan"]["grid"]].max()))[1] != G.VOCAB_OFF + 2:
        fails.append("tie: the key does not name the lower of the tied rows")
    # zeros: every row -|.|, row 5 = 0 * -1 = -0, row 40 = 0 * 1 = +0
    k = -np.abs(r.integers(1, 4, (nrows, K))) * np.sign(h).astype(np.int64)
    k[5] = k[40] = 0
    rs = np.ones(nrows, np.float32)
    rs[5] = -1.0
    out = _run_logits(torch, ops, xd, nwd, 0.0, _t(torch, k.astype(dt)), None, _t(torch, rs), nrows, cus, G.VOCAB_OFF)
    lg = out["logits"][:nrows]
    assert np.signbit(lg[5]) and lg[5] == 0 and not np.signbit(lg[40]) and lg[40] == 0 and (np.delete(lg, [5, 40]) < 0).all()
    _check_keys(fails, "zeros", out, nrows, G.VOCAB_OFF)
    if B.key_parts(int(out["keys"][:out["plan"]["grid"]].max()))[1] != G.VOCAB_OFF + 5:
        fails.append("zeros: -0 at the lower index must win against +0")
    _finish(fails)


def test_forced_plan_equals_automatic(gpu):
    """(e): cus = the device's compute units resolves the automatic plan and gives the same bits."""
    from simplellminference_amd import ops
    torch, fails = gpu, []
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    K, nrows = 2736, 333
    W, rs, Wv, _ = G.exact_weights(nrows, K, "i8", 3)
    x, nw = G.exact_x_norm(K, 3), G.exact_norm_w(K, 3)
    wd, xd, nwd, rsd = _t(torch, W), _t(torch, x), _t(torch, nw), _t(torch, rs)
    outs = [_run_logits(torch, ops, xd, nwd, 0.0, wd, None, rsd, nrows, c, 7) for c in (0, ncu)]
    grid = outs[0]["plan"]["grid"]
    assert {k: v for k, v in outs[0]["plan"].items() if k != "cus"} == {k: v for k, v in outs[1]["plan"].items() if k != "cus"}
    _same(fails, "auto", outs[0]["logits"], outs[1]["logits"], "logits differ between cus 0 and the device's count")
    _same(fails, "auto", outs[0]["keys"][:grid], outs[1]["keys"][:grid], "keys differ between cus 0 and the device's count")
    _hold(fails, "auto", outs[0]["logits"][:nrows], (Wv @ (x.astype(np.float64) * 0.25 * nw)) * rs, np.zeros(nrows))
    _finish(fails)
