"""The batched decode projections (simplellminference_amd/csrc/bgemm.h bgemm_kernel, bg_tile_kernel) one launch at a
time, through the kernel-level entry of sli.h ("batched decode stages, for tests and labs"), against the float64
reference tests/bgemm_ref.py (itself held to the C oracle by test_bgemm_ref_cpu.py). The entry launches the engine's
own code objects, and forces the plans a model of production size runs (test_batch_stage_cpu.py keeps the list of
forced plans, bgemm_ref.cells, covering every class the planner picks) on matrices of a few hundred rows.

Every output is filled with NaN sentinels before the launch; the q/k/v cache is three layers' worth of memory with
the middle layer under test. Each cell runs the row-major matrix and the fragment-layout image (tiled), which must
agree bit for bit (f).

Bars (derivations in bgemm_ref.py and prefill_ref.py next to each bound):
  (a) exact inputs (integer weights, power-of-two row scales and norm weights, x integers or a + c 2^-12 with a
      non-zero lo column; sum of absolute terms below 2^24 grid units, asserted): every partial sum is exact in fp32
      in any order. store: y == resid + sum * row scale * scale BIT FOR BIT, in place too. With a norm, sequence b's
      rows are fl32(fl32(sum * inv_b) * row scale) for ONE fp32 inv_b within 4 ulp of the float64 factor: recovered
      from the rows the epilogue leaves exact (q rows at position 0, v rows of an fp32 cache, every logits row), it
      must reproduce all of them; then k at position 0 and v in an fp16 / FP8 cache are the exact roundings of known
      fp32 values. RoPE at position > 0: prefill_ref.rope_tol; SwiGLU: act_tol less its hi/lo split terms; where
      inv_b could not be recovered (no exact row) it enters as 4.5 eps32 relative. fp16 cache: within_f16_rounding;
      FP8: the code of the reference, or its neighbour where ref +- tol straddles a boundary, under FLIP_CAP.
  (b) realistic inputs: sums within (4 eps32 sqrt(K) + 2^-22) (|W| @ |x w|) of the float64 sum of the same rounded
      operands, the fp32 norm factor within rtol 2e-6, both passed through each epilogue's derivative, plus (a).
  (c) keys: per sequence the maximum over keys_out[b][0 .. groups) names the value and the lowest index of the
      maximum of the kernel's own logits row (exact), with a planted tie across workgroups and -0 against +0.
  (d) nothing else is written: q / y / logits / act rows of sequences >= B, y / logits columns [nrows, ld), keys
      beyond [B][groups], every cache element but (b, head, pos[b]) of the middle layer.
  (e) two launches with splits > 1 on one workspace without clearing: both right, the counters zero after each.
  (f) tiled == row-major and forced plan == the same automatic plan, bit for bit.

Measured on an MI355X: every cell of (a) is bit-exact (the fp32 factor is recovered for every sequence that has an
exact row: all 408 per weight type with an fp32 cache, every logits row), no FP8 code needed its neighbour (0 of
101,376 per run) and (b) holds as stated, so no bar here was widened and nothing was found wrong in bgemm.h.

That it bites (scratch builds of bgemm.h with one arithmetic-only change each, not committed; this file run once per
build; tests failing of 22, and the bar that caught it first):
  1 lo column not added at the tile end      22  (a) store / logits / q rows of the "lo" family unequal (K 32 up)
  2 inv[b] not applied                       14  (a) no factor within 4 ulp reproduces the exact rows; act_tol
  3 sum of squares skips wave 0              14  (a) the same, from K 544 up (at K 32 the one block is wave 15's)
  4 row scale after the rotation              4  (a) int8 q / k at position > 0 outside rope_tol (v, fp16 pass)
  5 prefetched sin / cos for every item       0  equivalent, not a bug: a thread's items are 16 tiles apart, a whole
                                                 number of heads at hd 64 and 128 (128 pair rows), so they share d
                                                 and pos[b] and with them the table entry
  6 sigmoid where SiLU was asked              4  (a) act_mode 1 cells outside act_tol; (b)
  7 argmax key before the row scale           4  (c) int8 keys name another row than the logits' maximum; the tie
  8 tile kernel maps rows i >= 8 like i < 8   4  (f) gate/up tiled != row-major; (b)
"""
import functools

import numpy as np
import pytest

from tests import bgemm_ref as R
from tests import prefill_ref as P
from tests.test_gpu_prefill_kernels import _hold, _is_sentinel, _sentinel

pytestmark = pytest.mark.gpu

SENT8 = 0x7F                    # the FP8 NaN code: no finite value encodes to it
SENT64 = 0x7FC5A5A57FC5A5A5     # keys
POS = (0, R.T - 1, 17, 5, 23, 31, 11, 38)  # distinct; rotated per cell so the position-0 slot moves
BATCHES = (1, 3, 8)
INV_SLACK = 4.5 * R.EPS32       # an fp32 factor within 4 ulp of the float64 one, and the product's rounding
NORM = {"qkv": True, "gate_up": True, "store": False, "logits": True}


@pytest.fixture(scope="module")
def tables(gpu):
    """sin / cos tables [T][hd / 2] (device, and as numpy), per head_dim."""
    from simplellminference_amd import ops
    out = {}
    for hd in (64, 128):
        s, c = ops.rope_cache(hd, R.T, 10000.0)
        out[hd] = (s, c, s.cpu().numpy(), c.cpu().numpy())
        assert (out[hd][2][0] == 0).all() and (out[hd][3][0] == 1).all()  # position 0: the identity, exactly
    return out


def _t(torch, a):
    """A device copy of a numpy array (the cached cases are read-only and stay as they are)."""
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _shape_key(shape):
    return tuple(sorted(shape.items())) if isinstance(shape, dict) else shape


@functools.lru_cache(maxsize=None)
def _case_cached(role, skey, K, B, int8, kind):
    shape = dict(skey) if role == "qkv" else skey
    N = R.rows_of(role, shape)
    seed = 7 * K + 3 * N + B + (100 if int8 else 0)
    if kind == "real":
        W, scale, x, nw = R.real_inputs(N, K, B, int8, NORM[role], seed)
    else:
        W, scale, x, nw = R.exact_inputs(N, K, B, int8, kind, NORM[role], seed)
        assert R.exact_units(W, x, nw, kind) < 2 ** 24  # the condition of every bit-exact claim below
        if kind == "lo":
            assert R.lo_matters(W, x, nw) > 0.5, "dropping the lo column must change most outputs"
    Y, A = R.sums(W, x, nw)
    inv = R.inv_rms(x, R.EPS) if NORM[role] else None
    for a in (W, x, Y, A):
        a.setflags(write=False)
    return dict(W=W, scale=scale, x=x, nw=nw, Y=Y, A=A, inv=inv, N=N, K=K, B=B, exact=kind != "real")


def _case(role, shape, K, B, int8, kind):
    return _case_cached(role, _shape_key(shape), K, B, int8, kind)


def _same_bits(fails, tag, a, b):
    for k in a:
        if k == "plan":
            continue
        diff = a[k].view(np.uint8) != b[k].view(np.uint8)  # bytes: sentinels and NaNs compare
        if diff.any():
            fails.append(f"{tag}: {k} differs in {int(diff.sum())} bytes")


def _untouched(fails, tag, arr, written, what):
    """Everything outside the boolean mask `written` is still the sentinel."""
    if arr.dtype == np.uint8:
        sent = arr == SENT8
    elif arr.dtype == np.uint64:
        sent = arr == np.uint64(SENT64)
    else:
        sent = _is_sentinel(arr)
    bad = ~sent & ~written
    if bad.any():
        fails.append(f"{tag}: {int(bad.sum())} elements of {what} written outside their place, first at "
                     f"{np.argwhere(bad)[0].tolist()}")
    if written.any() and sent[written].any():
        fails.append(f"{tag}: {int(sent[written].sum())} elements of {what} not written")


# ---------------------------------------------------------------- launches
def _dev(torch, c):
    return _t(torch, c["x"]), _t(torch, c["nw"]), _t(torch, c["W"]), _t(torch, c["scale"])


def _run_store(torch, c, shape, plan, tiled, resid=None, in_place=False, scale=1.0, ws=None):
    from simplellminference_amd import ops
    nrows, ld = shape
    x, _, W, rs = _dev(torch, c)
    y = _sentinel(torch, (8, ld), False)
    r = None
    if resid is not None:
        if in_place:
            y[:c["B"], :nrows] = _t(torch, resid)
            r = y
        else:
            r = _sentinel(torch, (8, ld), False)
            r[:c["B"], :nrows] = _t(torch, resid)
    p = ops.batch_gemm_store(x, W, y, resid=r, scale=scale, row_scale=rs, tiled=tiled, plan=plan, ws=ws)
    return dict(y=y.cpu().numpy(), plan=p)


def _cache(torch, kv, shape):
    if kv == "f8":
        return torch.full(shape, SENT8, dtype=torch.uint8, device="cuda")
    return _sentinel(torch, shape, kv == "f16")


def _run_qkv(torch, tables, c, geo, kv, pos, plan, tiled):
    from simplellminference_amd import ops
    hq, hkv, hd = geo["hq"], geo["hkv"], geo["hd"]
    x, nw, W, rs = _dev(torch, c)
    B = c["B"]
    q = _sentinel(torch, (8, hq * hd), False)
    kc = _cache(torch, kv, (3, B, hkv, R.T, hd))
    vc = _cache(torch, kv, (3, B, hkv, R.T, hd))
    p = ops.batch_gemm_qkv(x, nw, R.EPS, W, q, kc[1], vc[1], _t(torch, np.asarray(pos, np.int32)), tables[hd][0],
                           tables[hd][1], hq, hkv, hd, row_scale=rs, tiled=tiled, plan=plan,
                           kv_dtype="f8" if kv == "f8" else None)
    k, v = kc.cpu().numpy(), vc.cpu().numpy()
    return dict(q=q.cpu().numpy(), k=k, v=v, plan=p)


def _run_gate_up(torch, c, inter, silu, plan, tiled):
    from simplellminference_amd import ops
    x, nw, W, rs = _dev(torch, c)
    act = _sentinel(torch, (8, inter), False)
    p = ops.batch_gemm_gate_up(x, nw, R.EPS, W, act, act_mode=silu, row_scale=rs, tiled=tiled, plan=plan)
    return dict(act=act.cpu().numpy(), plan=p)


def _run_logits(torch, c, shape, plan, tiled, scale=None):
    from simplellminference_amd import ops
    nrows, ld = shape
    x, nw, W, rs = _dev(torch, c)
    if scale is not None:
        rs = _t(torch, scale)
    groups = ops.batch_gemm_plan(nrows, c["K"], c["B"], True, plan=plan)[0]["groups"]
    logits = _sentinel(torch, (8, ld), False)
    keys = torch.full((8, groups + 3), SENT64, dtype=torch.int64, device="cuda")
    p = ops.batch_gemm_logits(x, nw, R.EPS, W, logits, keys, vocab_off=R.VOCAB_OFF, row_scale=rs, tiled=tiled, plan=plan)
    assert p["groups"] == groups
    return dict(logits=logits.cpu().numpy(), keys=keys.cpu().numpy().view(np.uint64), plan=p)


# ---------------------------------------------------------------- checks
def _known_rows(fails, tag, c, exact_rows):
    """a [B][N] as the kernel holds it and its uncertainty da. Exact inputs: exact_rows(b) -> (got values, column
    index) of the outputs the epilogue leaves exact for sequence b (or None); the fp32 factor is recovered from them
    and a is then known to the bit (da = 0). Otherwise, and for realistic inputs, the float64 a with its bound."""
    Y, inv, scale, B = c["Y"], c["inv"], c["scale"], c["B"]
    a = R.scaled(Y, inv, scale)
    if not c["exact"]:
        return a, R.scaled_tol(Y, R.sum_tol(c["A"], c["K"]), inv, scale), [False] * B
    assert R.is_f32(Y)
    a, da, known = a.copy(), INV_SLACK * np.abs(a), [False] * B
    for b in range(B):
        rows = exact_rows(b)
        if rows is None:
            continue
        got, cols = rows
        sc = None if scale is None else scale[cols]
        if not np.any(Y[b, cols] != 0):
            continue
        inv32 = R.recover_inv(np.asarray(got, np.float32), Y[b, cols], inv[b], sc)
        if inv32 is None:
            near = R.apply_inv(Y[b, cols], np.float32(inv[b]), sc)
            fails.append(f"{tag} seq {b}: no fp32 factor within 4 ulp of {inv[b]!r} reproduces its {len(cols)} exact "
                         f"outputs ({int((near != got).sum())} differ with the nearest, max |diff| "
                         f"{np.nanmax(np.abs(near.astype(np.float64) - got)):.3e})")
            continue
        a[b] = R.apply_inv(Y[b], inv32, scale).astype(np.float64)
        da[b] = 0.0
        known[b] = True
    return a, da, known


def _check_qkv(fails, tag, tables, out, c, geo, kv, pos, stats):
    hq, hkv, hd = geo["hq"], geo["hkv"], geo["hd"]
    _, _, sin_t, cos_t = tables[hd]
    B, nq, nk = c["B"], hq * hd, hkv * hd
    pos = np.asarray(pos)
    q, kc, vc = out["q"], out["k"], out["v"]
    sel = np.arange(B)
    got_k = kc[1][sel, :, pos, :]  # [B][hkv][hd]
    got_v = vc[1][sel, :, pos, :]

    def exact_rows(b):
        if pos[b] == 0:
            return q[b], np.arange(nq)
        if kv == "f32":
            return got_v[b].ravel(), np.arange(nq + nk, nq + 2 * nk)
        return None

    a, da, known = _known_rows(fails, tag, c, exact_rows)
    stats["recovered"] += sum(known)
    q_ref, k_ref, v_ref = R.epi_qkv(a, pos, sin_t, cos_t, hq, hkv, hd)
    tol_q = P.rope_tol(a[:, :nq], pos, sin_t, cos_t, hd, da[:, :nq])
    tol_k = P.rope_tol(a[:, nq:nq + nk], pos, sin_t, cos_t, hd, da[:, nq:nq + nk]).reshape(B, hkv, hd)
    tol_v = da[:, nq + nk:].reshape(B, hkv, hd).copy()
    for b in range(B):
        if pos[b] == 0:  # the identity: only the uncertainty of a itself remains
            tol_q[b] = da[b, :nq]
            tol_k[b] = da[b, nq:nq + nk].reshape(hkv, hd)
    _hold(fails, f"{tag} q", q[:B], q_ref, tol_q)
    for name, got, ref, tol in (("k", got_k, k_ref, tol_k), ("v", got_v, v_ref, tol_v)):
        if kv == "f16":
            ok = P.within_f16_rounding(got, ref, tol)
            if not ok.all():
                fails.append(f"{tag} {name} (fp16 cache): {int((~ok).sum())} of {ok.size} outside the rounding of ref +- tol")
        elif kv == "f8":
            ok, flip = R.f8_check(got, ref, tol)
            stats["f8"] += ok.size
            stats["f8_flips"] += int(flip.sum())
            if not ok.all():
                i = np.argwhere(~ok)[0]
                fails.append(f"{tag} {name} (FP8 cache): {int((~ok).sum())} of {ok.size} codes wrong, first at {i.tolist()}: "
                             f"got {got[tuple(i)]:#04x} for {ref[tuple(i)]!r} +- {tol[tuple(i)]:.2e}")
        else:
            _hold(fails, f"{tag} {name}", got, ref, tol)
    written = np.zeros(kc.shape, bool)
    written[1][sel, :, pos, :] = True
    _untouched(fails, tag, kc, written, "the K cache")
    _untouched(fails, tag, vc, written, "the V cache")
    wq = np.zeros(q.shape, bool)
    wq[:B] = True
    _untouched(fails, tag, q, wq, "q")


def _check_gate_up(fails, tag, out, c, inter, silu):
    B = c["B"]
    a, da, _ = _known_rows(fails, tag, c, lambda b: None)
    g, u = a[:, :inter], a[:, inter:]
    with np.errstate(over="ignore"):  # exp(-g) of the exact cases' large sums: the sigmoid saturates to 0
        ref, tol = P.act(g, u, silu), R.swiglu_tol(g, u, silu, da[:, :inter], da[:, inter:])
    _hold(fails, tag, out["act"][:B], ref, tol)
    w = np.zeros(out["act"].shape, bool)
    w[:B] = True
    _untouched(fails, tag, out["act"], w, "act")


def _check_store(fails, tag, out, c, shape, resid, scale):
    nrows, _ = shape
    B = c["B"]
    a = R.scaled(c["Y"], None, c["scale"])
    ref = R.epi_store(a, resid, scale)
    if c["exact"]:
        assert R.is_f32(ref)  # exact sums, grid residuals, power-of-two scales: no fp32 operation rounds
        tol = 0.0
    else:
        da = R.scaled_tol(c["Y"], R.sum_tol(c["A"], c["K"]), None, c["scale"])
        tol = da * abs(scale) + R.U32 * np.abs(a * scale) + R.U32 * np.abs(ref)
    _hold(fails, tag, out["y"][:B, :nrows], ref, tol)
    w = np.zeros(out["y"].shape, bool)
    w[:B, :nrows] = True
    _untouched(fails, tag, out["y"], w, "y")


def _check_keys(fails, tag, out, B, nrows):
    """(c): exact, from the kernel's own logits."""
    keys, groups = out["keys"], out["plan"]["groups"]
    for b in range(B):
        want = R.best_key(out["logits"][b, :nrows], R.VOCAB_OFF)
        got = int(keys[b, :groups].max())
        if got != want:
            (go, gi), (wo, wi) = R.key_parts(got), R.key_parts(want)
            fails.append(f"{tag} seq {b}: key names index {int(gi)} (image {int(go):#x}), the row's first maximum is at "
                         f"{int(wi)} (image {int(wo):#x})")
    w = np.zeros(keys.shape, bool)
    w[:B, :groups] = True
    _untouched(fails, tag, keys, w, "keys_out")


def _check_logits(fails, tag, out, c, shape, stats, scale=None):
    nrows, _ = shape
    B = c["B"]
    if scale is not None:
        c = dict(c, scale=scale)
    a, da, known = _known_rows(fails, tag, c, lambda b: (out["logits"][b, :nrows], np.arange(nrows)))
    stats["recovered"] += sum(known)
    _hold(fails, tag, out["logits"][:B, :nrows], a, da)
    w = np.zeros(out["logits"].shape, bool)
    w[:B, :nrows] = True
    _untouched(fails, tag, out["logits"], w, "logits")
    _check_keys(fails, tag, out, B, nrows)


def _plans_of(role):
    """The forced cells of bgemm_ref.cells(role) grouped by (shape, K), the automatic plan added once."""
    by = {}
    for shape, K, tpw, s in R.cells(role):
        by.setdefault((_shape_key(shape), K), [shape, []])[1].append((tpw, s))
    return [(shape, K, plans) for (_, K), (shape, plans) in by.items()]


def _expect_class(plan, tpw, s, K, norm):
    assert (plan["tpw"], plan["splits"]) == (tpw, s)
    per_wave = ((K // 32 + s - 1) // s + 15) // 16
    width = 2 if tpw == 1 else (7 if not norm and 6 <= per_wave <= 7 else 4)  # bgemm.h bg_launch_width
    assert plan["step_width"] == width, plan


# ---------------------------------------------------------------- (a) exact inputs, every forced plan
@pytest.mark.parametrize("w", ["f16", "i8"])
def test_store_exact_every_plan(gpu, w):
    """wo / down: y == resid + (sum * row scale) * scale bit for bit at every forced plan of bgemm_ref.cells("store")
    (widths 2, 4 and 7, short last workgroups, the wrap of the reducer wave, 1 to 4 splits), B in {1, 3, 8}, both x
    families; with a separate residual, none, and in place; tiled == row-major."""
    torch = gpu
    int8 = w == "i8"
    fails, n = [], 0
    for shape, K, plans in _plans_of("store"):
        for B in BATCHES:
            for kind in ("int", "lo"):
                c = _case("store", shape, K, B, int8, kind)
                resid = R.exact_resid(B, shape[0], K + B)
                for tpw, s in plans:
                    mode = n % 3  # 0: separate residual, scale 1/2; 1: in place, scale 2; 2: none
                    n += 1
                    kw = [dict(resid=resid, scale=0.5), dict(resid=resid, in_place=True, scale=2.0), dict()][mode]
                    tag = f"K {K} rows {shape[0]} B {B} {kind} plan {tpw}/{s} mode {mode}"
                    outs = [_run_store(torch, c, shape, (tpw, s), tiled, **kw) for tiled in (False, True)]
                    _expect_class(outs[0]["plan"], tpw, s, K, False)
                    _check_store(fails, tag, outs[0], c, shape, kw.get("resid"), kw.get("scale", 1.0))
                    _same_bits(fails, tag + " tiled vs row-major", outs[0], outs[1])
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("kv", ["f32", "f16", "f8"])
@pytest.mark.parametrize("w", ["f16", "i8"])
def test_qkv_exact_every_plan(gpu, tables, w, kv):
    """q/k/v: the fused norm's fp32 factor recovered per sequence from the exact rows and held to every one of them;
    k and v as the exact roundings of known values where it is; RoPE within its three roundings; nothing written
    but (b, head, pos[b]) of the middle layer. Every forced plan of bgemm_ref.cells("qkv"), B in {1, 3, 8}."""
    torch = gpu
    int8 = w == "i8"
    fails, n = [], 0
    stats = dict(recovered=0, f8=0, f8_flips=0)
    for shape, K, plans in _plans_of("qkv"):
        for B in BATCHES:
            for kind in ("int", "lo"):
                c = _case("qkv", shape, K, B, int8, kind)
                for tpw, s in plans:
                    pos = [POS[(i + n) % 8] for i in range(B)]
                    n += 1
                    tag = f"K {K} hd {shape['hd']} B {B} {kind} plan {tpw}/{s} pos {pos}"
                    outs = [_run_qkv(torch, tables, c, shape, kv, pos, (tpw, s), tiled) for tiled in (False, True)]
                    _expect_class(outs[0]["plan"], tpw, s, K, True)
                    _check_qkv(fails, tag, tables, outs[0], c, shape, kv, pos, stats)
                    _same_bits(fails, tag + " tiled vs row-major", outs[0], outs[1])
    print(f"qkv {w} {kv}: factor recovered for {stats['recovered']} sequences; FP8 neighbour codes "
          f"{stats['f8_flips']} of {stats['f8']}")
    assert stats["recovered"] > 0
    assert stats["f8_flips"] <= R.F8.FLIP_CAP * max(stats["f8"], 1)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("w", ["f16", "i8"])
def test_gate_up_exact_every_plan(gpu, w):
    """gate/up: sigmoid(g) u and SiLU(g) u within the activation's own fp32 roundings of exact sums (the norm factor
    to 4 ulp); act rows of sequences >= B untouched. Every forced plan, B in {1, 3, 8}, both x families."""
    torch = gpu
    int8 = w == "i8"
    fails, n = [], 0
    for shape, K, plans in _plans_of("gate_up"):
        for B in BATCHES:
            for kind in ("int", "lo"):
                c = _case("gate_up", shape, K, B, int8, kind)
                for tpw, s in plans:
                    silu = n % 2
                    n += 1
                    tag = f"K {K} inter {shape} B {B} {kind} plan {tpw}/{s} silu {silu}"
                    outs = [_run_gate_up(torch, c, shape, silu, (tpw, s), tiled) for tiled in (False, True)]
                    _expect_class(outs[0]["plan"], tpw, s, K, True)
                    _check_gate_up(fails, tag, outs[0], c, shape, silu)
                    _same_bits(fails, tag + " tiled vs row-major", outs[0], outs[1])
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("w", ["f16", "i8"])
def test_logits_exact_every_plan(gpu, w):
    """LM head: one fp32 factor per sequence reproduces every logits row bit for bit; the keys name the first
    maximum of the kernel's own row; columns [nrows, ld), rows >= B and keys beyond [B][groups] untouched. Every
    forced plan (the 8B head's class, 17 tiles per workgroup at K 4096, among them), B in {1, 3, 8}."""
    torch = gpu
    int8 = w == "i8"
    fails = []
    stats = dict(recovered=0)
    total = 0
    for shape, K, plans in _plans_of("logits"):
        for B in BATCHES:
            for kind in ("int", "lo"):
                if K == 4096 and shape[0] == R.NROWS_WIDE and (B, kind) not in ((8, "lo"), (3, "int")):
                    continue  # the one multi-MB matrix: two of the six (B, family) pairs
                c = _case("logits", shape, K, B, int8, kind)
                for tpw, s in plans:
                    tag = f"K {K} rows {shape[0]} B {B} {kind} plan {tpw}/{s}"
                    outs = [_run_logits(torch, c, shape, (tpw, s), tiled) for tiled in (False, True)]
                    _expect_class(outs[0]["plan"], tpw, s, K, True)
                    _check_logits(fails, tag, outs[0], c, shape, stats)
                    _same_bits(fails, tag + " tiled vs row-major", outs[0], outs[1])
                    total += B
    assert stats["recovered"] == total or fails, (stats, total)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# ---------------------------------------------------------------- (c) keys: ties and signed zeros
@pytest.mark.parametrize("w", ["f16", "i8"])
def test_keys_planted_tie_and_signed_zero(gpu, w):
    """Two equal maxima in tiles of different workgroups (rows 50 and 5, tpw 1; the lower index must win whichever
    workgroup stores first), and a row of zeros whose first element is -0.0 (a negative row scale on a zero sum): -0
    counts as +0, so index 0 wins."""
    torch = gpu
    int8 = w == "i8"
    shape, K, B = (R.NROWS, R.LD), 544, 3
    fails = []
    c = dict(_case("logits", shape, K, B, int8, "int"))
    W = c["W"].copy()
    h = R.staged(c["x"], c["nw"])[1]
    W[50] = W[5] = (np.sign(h) * 15).astype(W.dtype)  # sum = 15 sum |h|: above every other row of sequence 1
    c["W"] = W
    c["Y"], c["A"] = R.sums(W, c["x"], c["nw"])
    assert R.exact_units(W, c["x"], c["nw"], "int") < 2 ** 24
    scale = None if c["scale"] is None else c["scale"].copy()
    if scale is not None:
        scale[50] = scale[5] = 4.0
    a = R.scaled(c["Y"], c["inv"], scale)
    assert a[1, 5] == a[1, 50] == a[1].max() and (a[1] == a[1].max()).sum() == 2
    for plan in ((1, 1), (2, 1)):  # tiles 0 and 3: different workgroups either way
        out = _run_logits(torch, c, shape, plan, False, scale=scale)
        _check_logits(fails, f"tie plan {plan}", out, c, shape, dict(recovered=0), scale=scale)
        top = int(R.key_parts(out["keys"][1, :out["plan"]["groups"]].max())[1])
        if top != R.VOCAB_OFF + 5:
            fails.append(f"tie plan {plan}: sequence 1's key names {top}, not the lower of the two maxima {R.VOCAB_OFF + 5}")
    z = dict(_case("logits", shape, K, B, int8, "lo"))
    x = z["x"].copy()
    x[2] = 0.0
    z["x"] = x
    z["Y"], z["A"] = R.sums(z["W"], x, z["nw"])
    z["inv"] = R.inv_rms(x, R.EPS)
    zs = (np.ones(shape[0], np.float32) if z["scale"] is None else z["scale"].copy())
    zs[0] = -zs[0]
    zs[40] = -zs[40]
    out = _run_logits(torch, z, shape, (1, 1), True, scale=zs)
    row = out["logits"][2, :shape[0]]
    if not ((row == 0).all() and np.signbit(row[0]) and np.signbit(row[40]) and not np.signbit(row[1])):
        fails.append(f"signed zeros: sequence 2's row is not (-0, +0, ..): {row[:4]}")
    _check_logits(fails, "signed zeros", out, z, shape, dict(recovered=0), scale=zs)
    top = int(R.key_parts(out["keys"][2, :out["plan"]["groups"]].max())[1])
    if top != R.VOCAB_OFF:
        fails.append(f"signed zeros: sequence 2's key names {top}, not {R.VOCAB_OFF} (-0.0 must count as +0.0)")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- (b) realistic inputs
@pytest.mark.parametrize("w", ["f16", "i8"])
def test_realistic_values_every_role(gpu, tables, w):
    """N(0, 1) activations, N(0, 1/K) weights (int8: per-row symmetric, scale amax / 127), norm weights 1 + 0.1 N, at
    K 544 and 4096, B 3 and 8, plans 1/1 and 3/1 and the automatic one: bound (b) of the module docstring. The
    forced plan equal to the automatic one is bit-identical to it, as are the two layouts."""
    torch = gpu
    int8 = w == "i8"
    fails = []
    stats = dict(recovered=0, f8=0, f8_flips=0)
    from simplellminference_amd import ops
    for K in (544, 4096):
        for B in (3, 8):
            pos = [POS[(i + B) % 8] for i in range(B)]
            for role, shape in (("store", (R.NROWS, R.LD)), ("logits", (R.NROWS, R.LD)), ("gate_up", R.INTER),
                                ("qkv", R.QKV64), ("qkv", R.QKV128)):
                c = _case(role, shape, K, B, int8, "real")
                resid = np.random.default_rng(K + B).standard_normal((B, R.NROWS)).astype(np.float32)
                auto = ops.batch_gemm_plan(c["N"], K, B, NORM[role])[0]
                for what, plan in (("automatic", None), ("forced", (auto["tpw"], auto["splits"])), ("", (1, 1)), ("", (3, 1))):
                    tag = f"real {role} K {K} B {B} plan {plan}"
                    outs = []
                    for tiled in (False, True):
                        if role == "store":
                            outs.append(_run_store(torch, c, shape, plan, tiled, resid=resid, in_place=tiled))
                        elif role == "logits":
                            outs.append(_run_logits(torch, c, shape, plan, tiled))
                        elif role == "gate_up":
                            outs.append(_run_gate_up(torch, c, shape, 1, plan, tiled))
                        else:
                            outs.append(_run_qkv(torch, tables, c, shape, "f8" if shape is R.QKV128 else "f16", pos, plan,
                                                 tiled))
                    if role == "store":
                        _check_store(fails, tag, outs[0], c, shape, resid, 1.0)
                    elif role == "logits":
                        _check_logits(fails, tag, outs[0], c, shape, stats)
                    elif role == "gate_up":
                        _check_gate_up(fails, tag, outs[0], c, shape, 1)
                    else:
                        _check_qkv(fails, tag, tables, outs[0], c, shape, "f8" if shape is R.QKV128 else "f16", pos, stats)
                    _same_bits(fails, tag + " tiled vs row-major", outs[0], outs[1])
                    if what == "automatic":
                        first = outs[0]
                        assert {k: first["plan"][k] for k in auto} == auto
                    elif what == "forced":
                        _same_bits(fails, tag + " forced vs automatic", first, outs[0])
    print(f"realistic {w}: FP8 neighbour codes {stats['f8_flips']} of {stats['f8']}")
    assert stats["f8_flips"] <= R.F8.FLIP_CAP * max(stats["f8"], 1)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# ---------------------------------------------------------------- (e) workspace reuse across split launches
@pytest.mark.parametrize("w", ["f16", "i8"])
@pytest.mark.parametrize("K,plan", [(7168, (2, 2)), (1024, (1, 2)), (2816, (1, 4))])
def test_split_workspace_is_reused_without_clearing(gpu, w, K, plan):
    """Two launches with splits > 1 on one workspace, other inputs, nothing cleared in between: both exact, and the
    groups' arrival counters read zero after each (the last arriver resets them)."""
    torch = gpu
    shape = (R.NROWS, R.LD)
    fails = []
    ws = None
    for i, (B, kind) in enumerate(((8, "lo"), (3, "int"), (8, "int"))):
        c = _case("store", shape, K, B, w == "i8", kind)
        out = _run_store(torch, c, shape, plan, False, ws=ws)
        ws = out["plan"]["ws"]
        _check_store(fails, f"launch {i}", out, c, shape, None, 1.0)
        p = out["plan"]
        assert p["splits"] == plan[1] and p["counter_off"] > 0
        cnt = ws[p["counter_off"]:p["counter_off"] + 4 * p["groups"]].cpu().numpy().view(np.uint32)
        if cnt.any():
            fails.append(f"launch {i}: arrival counters {cnt.tolist()} after the launch")
    assert not fails, "\n".join(fails)
