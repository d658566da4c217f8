"""The GEMM prefill of a model with an FP8 E4M3 K/V cache (set_prefill("gemm-kv8"), SLI_PREFILL_GEMM_KV8): the
quantising q/k/v epilogue and the chunk attention over codes one launch at a time, the argument checks, the knob, and
the model path against the float64 FP8 reference.

Bars.
  1. The epilogue: the GEMM tiling is picked by (weight type, role, M), never by the cache type, so a launch into an
     fp32 cache and one into an FP8 cache compute the same fp32 values; the codes must be tests/kv8_ref.py's encode of
     the fp32 rows BIT FOR BIT and q identical.
  3. The attention widens the codes exactly to fp16 in registers, so what follows is the fp16 cache's arithmetic and
     the bar is test_gpu_prefill_kernels.py::test_prefill_attention_per_query's: 2e-6 + 1e-5 |ref| against float64
     attention on the decoded values.
  4. K = 0 makes every weight exactly 1 / (keys), the sums of <= 64 values that are multiples of 2^-9 below 2^14 are
     exact in fp32 in any order, so a row is the mean of V up to the division (1 / l, then the product: 1.5 x 2^-23)
     and the hi / lo split (2^-22): under rtol 1e-6.
  7. The model: the method of test_gpu_kv8.py::_model_against_reference with the project's bars (FLIP_CAP, logits
     1e-3, argmax where the top-2 gap exceeds 2e-3); the condition it rests on is checked without a GPU in
     tests/test_kv8_prefill_ref_cpu.py for these very token sequences.
"""
import ctypes

import numpy as np
import pytest

from tests import kv8_ref as K
from tests import prefill_ref as R
from tests.test_gpu_kv8 import _weights
from tests.test_gpu_prefill_kernels import POSITIONS, QKV, _bounds_cases
from tests.test_kv8_prefill_ref_cpu import PREFILL_RUNS, run_tokens

pytestmark = pytest.mark.gpu

SENT8 = 0x7F     # the NaN code: no finite value encodes to it
SENT32 = 0x7FC5A5A5


def _t(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def tables(gpu):
    """sin / cos tables [T][hd / 2] (device) for T = 528, per head_dim."""
    from simplellminference_amd import ops
    return {hd: ops.rope_cache(hd, 528, 10000.0) for hd in (64, 128)}


# ---------------------------------------------------------------- 1. the epilogue, bit for bit
def _wide_weights(torch, w, N, K_, seed):
    """Weights whose rows span 2^-16 .. 2^6 in magnitude, so with N(0, 1) activations the sums span 2^-13 .. 2^9:
    past 448 on one side and below the smallest subnormal 2^-9 on the other. Returns the keyword arguments of
    ops.prefill_gemm_qkv that carry them."""
    r = np.random.default_rng(seed)
    e = r.integers(-16, 7, N)
    if w == "f16":
        W = (r.standard_normal((N, K_)) * 2.0 ** e[:, None]).astype(np.float16)
        return _t(torch, W), {}
    if w == "i8":
        W = r.integers(-127, 128, (N, K_)).astype(np.int8)
        scale = (2.0 ** e / 64 * r.uniform(1, 2, N)).astype(np.float32)
        return _t(torch, W), {"row_scale": _t(torch, scale)}
    from tests import mxfp4_ref as mx
    codes = r.integers(0, 16, (N, K_)).astype(np.uint8)
    scales = np.repeat((127 + r.integers(-17, 5, (N, 1))).astype(np.uint8), K_ // 32, axis=1)  # one exponent per row
    return _t(torch, mx.pack(codes)), {"scales": _t(torch, scales)}


@pytest.mark.parametrize("w,hq,hkv,hd,K_,M", [(w, *s) for w in ("f16", "i8")
                                              for s in ((15, 3, 64, 128, 32), (15, 3, 64, 128, 256), (8, 2, 128, 64, 64))]
                         + [("mxfp4", 15, 3, 64, 128, 256)])
def test_qkv_epilogue_codes_bit_for_bit(gpu, tables, w, hq, hkv, hd, K_, M):
    torch = gpu
    from simplellminference_amd import ops
    N = (hq + 2 * hkv) * hd
    p0, T = 3, 3 + M + 8
    W, kw = _wide_weights(torch, w, N, K_, 100 * M + hd)
    x = np.random.default_rng(M + hd).standard_normal((M, K_)).astype(np.float32)
    hi, lo = ops.prefill_norm_split(_t(torch, x), None, 1e-5)
    sin_d, cos_d = tables[hd]
    out = {}
    for kv in ("f32", "f8"):
        q = torch.full((M, hq * hd), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
        if kv == "f32":
            kc = torch.full((hkv, T, hd), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
            vc = kc.clone()
            tl = ops.prefill_gemm_qkv(W, hi, lo, q, kc, vc, sin_d[:T], cos_d[:T], hq, hkv, hd, p0, M, **kw)
        else:
            kc = torch.full((hkv, T, hd), SENT8, dtype=torch.uint8, device="cuda")
            vc = kc.clone()
            tl = ops.prefill_gemm_qkv(W, hi, lo, q, kc, vc, sin_d[:T], cos_d[:T], hq, hkv, hd, p0, M, kv_dtype="f8", **kw)
        out[kv] = (q.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy(), tl)
    assert out["f32"][3] == out["f8"][3]  # one tiling
    assert np.array_equal(out["f32"][0].view(np.uint32), out["f8"][0].view(np.uint32)), "q differs"
    assert not np.isnan(out["f8"][0]).any()
    for which in (1, 2):
        rows32 = out["f32"][which][:, p0:p0 + M]
        codes = out["f8"][which][:, p0:p0 + M]
        a = np.abs(rows32)
        assert (a > 448).mean() > 0.01 and ((a > 0) & (a < 2.0 ** -9)).mean() > 0.01, "the inputs miss the edges"
        want = K.encode(rows32)
        bad = np.argwhere(codes != want)
        assert bad.size == 0, (f"{'qkv'[which]}: {len(bad)} of {codes.size} codes differ, first at {bad[0].tolist()}: "
                               f"{rows32[tuple(bad[0])]!r} -> {codes[tuple(bad[0])]:#04x}, want {want[tuple(bad[0])]:#04x}")
        rest = np.ones(T, bool)
        rest[p0:p0 + M] = False
        assert (out["f8"][which][:, rest] == SENT8).all()


# ---------------------------------------------------------------- 2. the stores stay in their rows
@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("M", [64, 256])
def test_qkv_f8_cache_stores_stay_in_their_rows(gpu, tables, M, case):
    """The (p0, nv, T) cases of test_gpu_prefill_kernels.py on an FP8 cache filled with the NaN code, with guard bytes
    in front of and behind the allocation the kernel is given: afterwards exactly rows p0 .. p0 + nv - 1 below T hold
    codes (none of them the NaN code), every other byte is the sentinel."""
    torch = gpu
    from simplellminference_amd import ops
    p0, nv, T = _bounds_cases(M)[case]
    hq, hkv, hd = QKV["hq"], QKV["hkv"], QKV["hd"]
    N = (hq + 2 * hkv) * hd
    W, _, hi, lo = R.grid_inputs(N, 128, M, False, 7 + case)
    sin_d, cos_d = tables[hd]
    guard, n = 4096, hkv * T * hd
    bufs = [torch.full((guard + n + guard,), SENT8, dtype=torch.uint8, device="cuda") for _ in range(2)]
    kc, vc = (b[guard:guard + n].view(hkv, T, hd) for b in bufs)
    q = torch.zeros((M, hq * hd), dtype=torch.float32, device="cuda")
    ops.prefill_gemm_qkv(_t(torch, W), _t(torch, hi), _t(torch, lo), q, kc, vc, sin_d[:T], cos_d[:T], hq, hkv, hd, p0,
                         nv, kv_dtype="f8")
    rows = np.arange(p0, min(p0 + nv, T))
    assert rows.size > 0
    for name, b in zip("kv", bufs):
        b = b.cpu().numpy()
        assert (b[:guard] == SENT8).all() and (b[guard + n:] == SENT8).all(), f"{name}: guard bytes written"
        c = b[guard:guard + n].reshape(hkv, T, hd)
        inside = np.zeros(T, bool)
        inside[rows] = True
        assert (c[:, ~inside] == SENT8).all(), f"{name}: rows outside {p0}..{p0 + nv - 1} (below {T}) written"
        assert ((c[:, inside] & 0x7F) != SENT8).all(), f"{name}: a row inside holds the sentinel"


# ---------------------------------------------------------------- 3. the attention, per query
ATTN_POSITIONS = POSITIONS + [(0, 256, 256),   # all 16 row groups; the last has 8 tiles, two per wave
                              (224, 32, 256)]  # a chunk's tail against a full cache


def _attn_case(hd, hq, hkv, p0, M, T):
    r = np.random.default_rng(p0 + M + T + hd + hq)
    q = r.standard_normal((M, hq * hd)).astype(np.float32)
    kq = K.encode(r.standard_normal((hkv, T, hd)).astype(np.float32))
    vq = K.encode(r.standard_normal((hkv, T, hd)).astype(np.float32))
    return q, kq, vq


@pytest.mark.parametrize("p0,M,T", ATTN_POSITIONS)
@pytest.mark.parametrize("hd,hq,hkv", [(hd, hq, hkv) for hd in (64, 128) for hq, hkv in ((2, 2), (8, 2))])
def test_prefill_attention_f8_per_query(gpu, hd, hq, hkv, p0, M, T):
    torch = gpu
    from simplellminference_amd import ops
    q, kq, vq = _attn_case(hd, hq, hkv, p0, M, T)
    ohi, olo = ops.prefill_attn(_t(torch, q), _t(torch, kq), _t(torch, vq), M, p0, hq, hkv, hd, kv_dtype="f8")
    got = R.joined(ohi.cpu().numpy(), olo.cpu().numpy())
    ref = R.attn(q, K.decode(kq), K.decode(vq), p0, hq, hkv, hd, rows=M)
    n = min(M, T - p0)
    assert n > 0 and not np.isnan(ref[:n]).any()
    err = np.abs(got[:n] - ref[:n])
    lim = 2e-6 + 1e-5 * np.abs(ref[:n])
    print(f"hd {hd} hq {hq} hkv {hkv} p0 {p0} M {M} T {T}: max err {err.max():.3e}, worst err / lim {(err / lim).max():.3f}")
    assert np.all(err <= lim), f"max err {err.max():.3e}, worst excess {(err - lim).max():.3e}"
    if (p0, M, T, hd, hq) == (0, 64, 64, 64, 2):  # the same bytes as a float8_e4m3fn tensor
        f8 = torch.float8_e4m3fn
        ohi8, olo8 = ops.prefill_attn(_t(torch, q), _t(torch, kq).view(f8), _t(torch, vq).view(f8), M, p0, hq, hkv, hd)
        assert torch.equal(ohi, ohi8) and torch.equal(olo, olo8)


# ---------------------------------------------------------------- 4. extreme codes
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("p0,M", [(0, 64), (32, 32)])
def test_prefill_attention_f8_extreme_codes(gpu, hd, p0, M):
    """As test_gpu_kv8.py::test_mha_f8_extreme_values_decode: K all zero, V rows of +-448 and +-2^-9 (the largest value
    and the smallest subnormal), so chunk row m is the mean of V over keys 0 .. p0 + m.
    The rows come in the order 448, 2^-9, -2^-9, -448 (odd columns and kv head 1 with the signs swapped), so a prefix
    sum is 0, +-448 or +-(448 + 2^-9) and every mean is 0 or at least 448 / 64: the result leaves the kernel as an
    fp16 hi + lo pair, which carries a value no finer than 2^-25 absolute (prefill_ref.SPLIT_ABS), so a mean such as
    2^-9 / 3 cannot be held to 1e-6 relative by any kernel with that output (the first layout tried had such prefixes:
    7.6e-4). Losing a 2^-9 beside 448 is 4.4e-6 relative, which the bar still sees."""
    torch = gpu
    from simplellminference_amd import ops
    T, hq, hkv = 64, 4, 2
    q = np.ones((M, hq * hd), np.float32)
    kq = np.zeros((hkv, T, hd), np.uint8)
    vq = np.empty((hkv, T, hd), np.uint8)
    for t in range(T):
        vq[:, t] = (0x7E, 0x01, 0x81, 0xFE)[t % 4]
    vq[:, :, 1::2] ^= 0x80
    vq[1] ^= 0x80
    ohi, olo = ops.prefill_attn(_t(torch, q), _t(torch, kq), _t(torch, vq), M, p0, hq, hkv, hd, kv_dtype="f8")
    got = R.joined(ohi.cpu().numpy(), olo.cpu().numpy()).reshape(M, hq, hd)
    V = K.decode(vq).astype(np.float64)
    mean = np.cumsum(V, axis=1) / np.arange(1, T + 1)[None, :, None]  # [hkv][t][hd]: the mean of keys 0 .. t
    want = np.stack([mean[h // (hq // hkv), p0:p0 + M] for h in range(hq)], axis=1)
    assert np.unique(want).size >= 3
    err = np.abs(got - want)
    assert np.all(err <= 1e-6 * np.abs(want)), f"max relative error {np.nanmax(err / np.abs(want)):.3e}"
    if p0 == 0:  # a subnormal alone survives (nothing flushes it): one live key holding +-2^-9
        vq1 = np.full((hkv, T, hd), 0x01, np.uint8)
        vq1[:, :, 1::2] = 0x81
        ohi, olo = ops.prefill_attn(_t(torch, q), _t(torch, kq), _t(torch, vq1), M, 0, hq, hkv, hd, kv_dtype="f8")
        row0 = R.joined(ohi.cpu().numpy(), olo.cpu().numpy())[0]
        assert np.array_equal(row0, np.tile(np.array([2.0 ** -9, -2.0 ** -9]), hq * hd // 2))


# ---------------------------------------------------------------- 5. argument checks
def test_prefill_attn_f8_argument_checks(gpu):
    """The refusals launch nothing; the one good call between them shows that each refusal is about the argument it
    names."""
    torch = gpu
    from simplellminference_amd import _lib
    L = _lib.load()
    M, T, hq, hkv, hd = 64, 64, 2, 1, 64
    q = torch.zeros(M * hq * hd, dtype=torch.float32, device="cuda")
    c8 = torch.zeros(hkv * T * hd + 64, dtype=torch.uint8, device="cuda")
    ohi = torch.zeros(M * hq * hd, dtype=torch.float16, device="cuda")
    olo = torch.zeros_like(ohi)
    st = torch.zeros(48, dtype=torch.int32, device="cuda")  # SLI_PF_TABLE_BYTES
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    F8, ARG = _lib.DT_F8E4M3, 1

    def attn(dt=F8, kp=None, vp=None, M_=M, rows=M):
        return L.sli_prefill_attn(p(q), p(c8) if kp is None else kp, p(c8) if vp is None else vp, dt, p(ohi), p(olo), M_,
                                  rows, 0, hq, hkv, hd, T, p(st), None)

    assert attn() == 0
    assert attn(kp=p(c8, 8)) == ARG     # every DMA piece is 16 bytes of a row
    assert attn(vp=p(c8, 4)) == ARG
    assert attn(dt=_lib.DT_I8) == ARG   # no such cache
    assert attn(rows=M - 1) == ARG      # the MFMA kernel touches M rows of q / ohi / olo
    assert attn(M_=48, rows=64) == ARG  # not a chunk size
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. the knob
def test_prefill_mode_knob_kv8(gpu):
    from simplellminference_amd._lib import SliError
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    cfg = preset("tiny-gqa")
    m8 = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f8", seed=0).init()
    assert m8.prefill_path() == "decode"  # the default
    with pytest.raises(SliError) as e:
        m8.set_prefill("gemm")
    assert e.value.code == 7 and "cannot take the GEMM prefill" in str(e.value)
    assert m8.prefill_path() == "decode"
    for mode, path in (("gemm-kv8", "mfma"), ("decode", "decode"), ("gemm-kv8", "mfma"), ("auto", "decode"),
                       ("gemm-kv8", "mfma")):
        m8.set_prefill(mode)
        assert m8.prefill_path() == path, (mode, m8.prefill_path())
    m8.close()
    prompt = [int(t) for t in np.random.default_rng(3).integers(1, cfg.vocab_size, 33)]
    m16 = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=0).init()
    m16.set_prefill("gemm")
    a = m16.predict_prefill(prompt, 48)
    m16.reset()
    m16.set_prefill("gemm-kv8")  # SLI_PREFILL_GEMM for every model that is not an FP8-cache one
    assert m16.prefill_path() == "mfma"
    assert np.array_equal(a, m16.predict_prefill(prompt, 48))
    m16.close()
    f = LlamaModel(config=cfg, w_dtype="f32", kv_dtype="f32", seed=0).init()
    with pytest.raises(SliError) as e:
        f.set_prefill("gemm-kv8")
    assert e.value.code == 7 and f.prefill_path() == "decode"
    f.close()
    g = TPGroup(cfg, 2, w_dtype="f16", kv_dtype="f8", seed=0).init()
    assert g.prefill_path() == "decode"
    g.set_prefill("gemm-kv8")
    assert g.prefill_path() == "mfma"
    g.close()


# ---------------------------------------------------------------- 7. the model against the float64 FP8 reference
def _prefill_run(make, toks, k):
    """A fresh model from make(): toks[:k] prefilled under "gemm-kv8" (positions 0 .. k - 2 through the GEMM path),
    then toks[k - 1:] teacher-forced one decode step at a time. Returns the logits [n, V] (rows below k - 1 NaN) and
    the K / V rows [L][which] -> [n, KV] (a TPGroup's shards concatenated by kv head)."""
    gm = make()
    ranks = getattr(gm, "ranks", [gm])
    n = len(toks)
    gm.set_prefill("gemm-kv8")
    assert gm.prefill_path() == "mfma"
    gm.prefill(toks[:k])
    logits = np.full((n, ranks[0].config.vocab_size), np.nan, np.float32)
    for p in range(k - 1, n):
        for m in ranks:
            m.set_state_seq(0, int(toks[p]), p, advance=False)
        gm.step()
        lg = gm.logits()
        logits[p] = lg if len(ranks) > 1 else lg[0]
    assert all(m.state()["error"] == 0 for m in ranks)
    L = ranks[0].config.num_hidden_layers
    rows = [[np.concatenate([m.kv(l, which, n) for m in ranks], axis=1) for which in (0, 1)] for l in range(L)]
    gm.close()
    return logits, rows


def _prefill_against_reference(oracle, name, w_dtype, seed, k, n, make, what):
    from simplellminference_amd.model import preset
    cfg = preset(name)
    oc, W = _weights(oracle, name, seed, w_dtype)
    toks = run_tokens(cfg, n)
    _, rows32 = _prefill_run(lambda: make("f32"), toks, k)
    logits8, rows8 = _prefill_run(lambda: make("f8"), toks, k)
    rows64, _ = K.unrounded_rows(oc, W, toks)
    slack = K.slack_from(rows64, lambda l, p, which: rows32[l][which][p])
    for kv in rows8:  # what the cache returns is on the FP8 grid
        for r in kv:
            assert np.array_equal(K.decode(K.encode(r)), r)
    codes = [[K.encode(r) for r in kv] for kv in rows8]
    ref, w = K.walk_run(oc, W, toks, lambda l, p, which: codes[l][which][p], slack)
    K.check_flips(w, what)
    K.check_logits(logits8[k - 1:], ref[k - 1:], what)


@pytest.mark.parametrize("name,w_dtype,seed,k,n", PREFILL_RUNS)
def test_model_gemm_kv8_prefill(gpu, oracle, name, w_dtype, seed, k, n):
    """64-row bucket at hd 64 (GQA, MHA, MXFP4 weights); small-h128-gqa: a full 256-row chunk plus a 43-row tail in
    the 64 bucket, hd 128, GQA-2, keys past one tile per wave."""
    from simplellminference_amd.model import LlamaModel, preset
    make = lambda kv: LlamaModel(config=preset(name), w_dtype=w_dtype, kv_dtype=kv, seed=seed).init()
    _prefill_against_reference(oracle, name, w_dtype, seed, k, n, make, f"{name} {w_dtype} gemm-kv8 prefill {k} of {n}")


def test_tp_group_gemm_kv8_prefill(gpu, oracle):
    from simplellminference_amd.model import TPGroup, preset
    name, w_dtype, seed, k, n = PREFILL_RUNS[0]
    make = lambda kv: TPGroup(preset(name), 2, w_dtype=w_dtype, kv_dtype=kv, seed=seed).init()
    _prefill_against_reference(oracle, name, w_dtype, seed, k, n, make, f"{name} {w_dtype} TP-2 group gemm-kv8 prefill")
