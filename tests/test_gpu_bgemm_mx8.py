"""The batched decode projection on the block-scaled MFMA (csrc/bgemm_mx8.h, sli_batch_gemm_mx8): FP4 weights times
MXFP8 activations that the launch quantises while it stages them. The launch restatement, epilogue checks and bounds are
tests/bgemm_ref.py's and tests/test_gpu_batch_kernels.py's, over the dequantised weights (tests/bgemm_mx_ref.py) and the
activations as the numpy rule of the format quantises them (tests/mx8_ref.py).

Plans are (tpw, splits, wt, wk): wk 16 / 4 / 1 k-slices (the 16-way reduce, a 4-way reduce under 4 tiles in flight, no
reduce and the wave's own epilogue stores), tpw 3 and 5 leave a short last workgroup and a round with idle tile lanes,
splits 2 runs the write-through hand-off. K 128: one stage (15 of 16 slices empty); 384: an odd stage count; 1024: 8
stages, more than 4 slices hold and fewer than 16.
"""
import functools

import numpy as np
import pytest

from tests import bgemm_mx_ref as M
from tests import bgemm_ref as R
from tests import mx8_ref
from tests import mxfp4_ref as mx
from tests import test_gpu_batch_kernels as BK

pytestmark = pytest.mark.gpu
tables = BK.tables  # the module-scoped sin / cos tables fixture

PLANS = ((1, 1, 1, 16), (3, 1, 4, 4), (5, 1, 16, 1), None)
SPLIT_PLANS = ((2, 2, 4, 4), (3, 2, 16, 1))  # roles without a norm, K >= 256
SHAPES = {"qkv": (dict(hq=1, hkv=1, hd=64), R.QKV64), "gate_up": (8, R.INTER), "store": ((16, 16), (100, 112)),
          "logits": ((16, 16), (100, 112))}


def _t(torch, a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _finish(W, x, nw, norm, codes, scales, exact):
    """A bgemm_ref case dict whose sums are float64 over the activations as MXFP8 holds them."""
    h8 = mx8_ref.dequantize(*mx8_ref.quantize(R.staged(x, nw)))
    Y, A = h8 @ W.T, np.abs(h8) @ np.abs(W).T
    N, K = W.shape
    return dict(W=W, scale=None, x=x, nw=nw, Y=Y, A=A, inv=R.inv_rms(x, R.EPS) if norm else None, N=N, K=K, B=x.shape[0],
                exact=exact, data=mx.pack(codes), scales=scales, h8=h8)


@functools.lru_cache(maxsize=None)
def _exact_case(N, K, B, norm):
    """Every e2m1 code, scale bytes 126..128; x * norm_w an integer |.| <= 8 times a per-block 2^-1..2^1, which e4m3
    holds exactly under the block's scale. Terms are multiples of 2^-3 and |sum| <= K * 6 * 2 * 16 < 2^24 * 2^-3 at K
    1024, so every partial sum is an fp32 number in any order."""
    r = np.random.default_rng(13 * K + 7 * N + B)
    codes = r.integers(0, 16, (N, K)).astype(np.uint8)
    scales = r.integers(126, 129, (N, K // 32)).astype(np.uint8)
    nw = (2.0 ** r.integers(0, 2, K)).astype(np.float32) if norm else None
    lim = 8 if nw is None else (8 // nw.astype(np.int64))[None, :]
    x = r.integers(-8, 9, (B, K)).clip(-lim, lim).astype(np.float32)
    x *= np.repeat(2.0 ** r.integers(-1, 2, (B, K // 32)), 32, axis=1).astype(np.float32)
    c = _finish(M.dequant64(codes, scales), x, nw, norm, codes, scales, True)
    assert np.array_equal(c["h8"], R.staged(x, nw).astype(np.float64))  # the quantiser is exact on these
    assert R.is_f32(c["Y"]) and c["A"].max() * 8 < 2 ** 24
    return c


def _run(torch, tables, role, c, shape, plan, tiled, kv="f32", pos=None, silu=0, resid=None):
    from simplellminference_amd import ops
    x, nw, data, sc = (_t(torch, c[k]) for k in ("x", "nw", "data", "scales"))
    kw = dict(tiled=tiled, plan=plan, scales=sc)
    if role == "store":
        y = BK._sentinel(torch, (8, shape[1]), False)
        r = None
        if resid is not None:
            r = BK._sentinel(torch, (8, shape[1]), False)
            r[:c["B"], :shape[0]] = _t(torch, resid)
        p = ops.batch_gemm_store_mx8(x, data, y, resid=r, **kw)
        return dict(y=y.cpu().numpy(), plan=p)
    if role == "gate_up":
        act = BK._sentinel(torch, (8, shape), False)
        p = ops.batch_gemm_gate_up_mx8(x, nw, R.EPS, data, act, act_mode=silu, **kw)
        return dict(act=act.cpu().numpy(), plan=p)
    if role == "logits":
        groups = ops.batch_gemm_mx8_plan(shape[0], c["K"], c["B"], True, plan=plan)[0]["groups"]
        logits = BK._sentinel(torch, (8, shape[1]), False)
        keys = torch.full((8, groups + 3), BK.SENT64, dtype=torch.int64, device="cuda")
        p = ops.batch_gemm_logits_mx8(x, nw, R.EPS, data, logits, keys, vocab_off=R.VOCAB_OFF, **kw)
        assert p["groups"] == groups
        return dict(logits=logits.cpu().numpy(), keys=keys.cpu().numpy().view(np.uint64), plan=p)
    hq, hkv, hd = shape["hq"], shape["hkv"], shape["hd"]
    q = BK._sentinel(torch, (8, hq * hd), False)
    kc, vc = (BK._cache(torch, kv, (3, c["B"], hkv, R.T, hd)) for _ in range(2))
    p = ops.batch_gemm_qkv_mx8(x, nw, R.EPS, data, q, kc[1], vc[1], _t(torch, np.asarray(pos, np.int32)), tables[hd][0],
                               tables[hd][1], hq, hkv, hd, kv_dtype="f8" if kv == "f8" else None, **kw)
    return dict(q=q.cpu().numpy(), k=kc.cpu().numpy(), v=vc.cpu().numpy(), plan=p)


def _check(fails, tag, tables, role, out, c, shape, stats, kv="f32", pos=None, silu=0, resid=None):
    if role == "store":
        BK._check_store(fails, tag, out, c, shape, resid, 1.0)
    elif role == "gate_up":
        BK._check_gate_up(fails, tag, out, c, shape, silu)
    elif role == "logits":
        BK._check_logits(fails, tag, out, c, shape, stats)
    else:
        BK._check_qkv(fails, tag, tables, out, c, shape, kv, pos, stats)


# ---------------------------------------------------------------- 1. exact sums, bit for bit
@pytest.mark.parametrize("K", [128, 384, 1024])
@pytest.mark.parametrize("role,kv", [("store", "f32"), ("gate_up", "f32"), ("logits", "f32"), ("qkv", "f32"),
                                     ("qkv", "f16"), ("qkv", "f8")])
def test_exact(gpu, tables, role, kv, K):
    torch = gpu
    norm = BK.NORM[role]
    fails, n = [], 0
    stats = dict(recovered=0, f8=0, f8_flips=0)
    for shape in SHAPES[role]:
        N = R.rows_of(role, shape)
        for B in (1, 3, 8):
            c = _exact_case(N, K, B, norm)
            for plan in PLANS + (SPLIT_PLANS if not norm and K >= 256 else ()):
                n += 1
                kw = dict(kv=kv, pos=[BK.POS[(i + n) % 8] for i in range(B)], silu=n % 2,
                          resid=R.exact_resid(B, shape[0], K + B) if role == "store" and n % 2 else None)
                tag = f"{role} {kv} K {K} N {N} B {B} plan {plan}"
                outs = [_run(torch, tables, role, c, shape, plan, tiled, **kw) for tiled in (False, True)]
                p = outs[0]["plan"]
                assert p["wt"] * p["wk"] == 16 and (plan is None or (p["tpw"], p["splits"], p["wt"], p["wk"]) == plan)
                _check(fails, tag, tables, role, outs[0], c, shape, stats, **kw)
                BK._same_bits(fails, tag + " tiled vs row-major", outs[0], outs[1])
    assert stats["f8_flips"] <= R.F8.FLIP_CAP * max(stats["f8"], 1)
    assert role in ("store", "gate_up") or stats["recovered"] > 0
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


# ---------------------------------------------------------------- 2. the staged image, through one-hot weights
@pytest.mark.parametrize("spread", [0, 20])
@pytest.mark.parametrize("K", [128, 256])
def test_staged_image(gpu, tables, K, spread):
    """W = identity (code 1.0, scale byte 127): y[b][r] is element r of the staged image, dequantised. Store: x itself,
    no allowance. Logits: x * norm_w, times the fp32 1/rms recovered within 4 ulp (bgemm_ref.recover_inv)."""
    torch = gpu
    r = np.random.default_rng(K + spread)
    codes = np.where(np.eye(K, dtype=bool), 2, 0).astype(np.uint8)
    scales = np.full((K, K // 32), 127, np.uint8)
    x = r.standard_normal((8, K)).astype(np.float32)
    x *= np.repeat(2.0 ** r.integers(-spread, spread + 1, (8, K // 32)), 32, axis=1).astype(np.float32)
    nw = r.uniform(0.5, 1.5, K).astype(np.float32)
    fails, stats = [], dict(recovered=0)
    for role, plan in (("store", (1, 1, 1, 16)), ("store", (3, 1, 16, 1)), ("logits", (2, 1, 4, 4)), ("logits", None)):
        norm = role == "logits"
        c = _finish(M.dequant64(codes, scales), x, nw if norm else None, norm, codes, scales, True)
        assert np.array_equal(c["Y"], c["h8"])
        out = _run(torch, tables, role, c, (K, K), plan, False)
        _check(fails, f"{role} K {K} spread {spread} plan {plan}", tables, role, out, c, (K, K), stats)
    assert stats["recovered"] == 16 or fails
    assert not fails, "\n".join(fails[:30])


# ---------------------------------------------------------------- 3. realistic values
@pytest.mark.parametrize("K", [512, 4096])
@pytest.mark.parametrize("role", ["store", "logits"])
def test_realistic(gpu, tables, role, K):
    """|err| <= (2^-16 + P 2^-24) (|W| @ |A|): 2^-16 the recorded never-exceed of one issue's internal sum, P
    the fp32 partials added per output: stages per k-slice + wk + splits. Worst ratios measured: see DESIGN.md §4."""
    torch = gpu
    from simplellminference_amd import ops
    norm = role == "logits"
    quant = lambda wf: tuple(t.cpu().numpy() for t in ops.quant_mxfp4(_t(torch, wf)))
    base = M.real_case(100, K, 8, norm, K + norm, quant)
    c = _finish(base["W"], base["x"], base["nw"], norm, base["codes"], base["scales"], False)
    worst = 0.0
    for plan in ((2, 1, 4, 4), None) + (((1, 2, 1, 16),) if not norm else ()):
        out = _run(torch, tables, role, c, (100, 112), plan, True)
        p = out["plan"]
        P = -(-(K // 128) // (p["splits"] * p["wk"])) + p["wk"] + p["splits"]
        dY = (2.0 ** -16 + P * 2.0 ** -24) * c["A"]
        got = out["y" if role == "store" else "logits"][:8, :100].astype(np.float64)
        ref, tol = R.scaled(c["Y"], c["inv"], None), R.scaled_tol(c["Y"], dY, c["inv"], None)
        err = np.abs(got - ref)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        print(f"{role} K {K} plan {p['tpw']}/{p['splits']}/{p['wt']}x{p['wk']}: worst err / bound {worst:.3f}")
        assert (err <= tol).all(), (role, K, plan, worst)


# ---------------------------------------------------------------- 4. the weights' scale range
@pytest.mark.parametrize("tiled", [False, True])
def test_scale_range(gpu, tables, tiled):
    """Scale bytes 1..254 (bgemm_mx_ref.scale_range_case) and byte 0 in row 0, against one-hot activations of 256 (amax 2^8:
    the block's scale byte is 127, its code 256): y[b][r] = 256 W[r][c_b] wherever that is a normal fp32 number."""
    torch = gpu
    codes, scales = M.scale_range_case()
    scales = scales.copy()
    scales[0, :] = 0
    N, K = codes.shape
    cols = [0, 37, 70, 101, 140, 171, 202, 255]  # a different block per sequence
    x = np.zeros((8, K), np.float32)
    x[np.arange(8), cols] = 256.0
    assert (mx8_ref.quantize(x)[1] == 127).all()
    W = np.ldexp(mx.GRID.astype(np.float64)[codes & 7] * np.where(codes & 8, -1.0, 1.0),
                 np.repeat(scales.astype(np.int64) - 127, 32, axis=1))
    c = _finish(W, x, None, False, codes, scales, False)
    out = _run(torch, tables, "store", c, (N, N), None, tiled)["y"][:8, :N]
    ref = c["Y"]
    ok = (np.abs(ref) <= np.finfo(np.float32).max) & ((np.abs(ref) >= 2.0 ** -126) | (ref == 0))
    assert ok.mean() > 0.9
    bad = ok & (out.astype(np.float64) != ref)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
