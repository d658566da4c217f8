"""The FP8 E4M3 K/V cache (SLI_DT_F8E4M3) on the GPU: the quantiser bit for bit, the MFMA decode attention over an
FP8 cache against the oracle's attention on the decoded values, the argument checks, and the model path.

Bars. The quantiser and the decode are exact (tests/kv8_ref.py is the rule of include/sli.h). The attention widens
the codes exactly to fp16 in registers, so what follows is the fp16 cache's arithmetic and the bar is
test_gpu_ops.py::test_mha's: rtol 1e-5, atol 2e-6 against the oracle on the decoded fp32 cache.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import kv8_ref as K
from tests.test_kv8_ref_cpu import f8_inputs

pytestmark = pytest.mark.gpu


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, want, rtol, atol):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    err = np.abs(got - want)
    lim = atol + rtol * np.abs(want)
    assert np.all(err <= lim), f"max err {err.max():.3e} (worst excess {(err - lim).max():.3e})"


# ---------------------------------------------------------------- 1. the quantiser, bit for bit
def test_quant_f8_bit_for_bit(gpu):
    from simplellminference_amd import ops
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    dn = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    extra = np.array([448, -448, up(448), -up(448), 464, -464, 465, -465, 1e9, -1e9, np.inf, -np.inf, np.nan, 0.0, -0.0,
                      2.0 ** -10, up(2.0 ** -10), dn(2.0 ** -10), -2.0 ** -10, -up(2.0 ** -10), -dn(2.0 ** -10),
                      3e38, 1e-40, -1e-40], np.float32)
    x = np.concatenate([f8_inputs(), extra])
    got = ops.quant_f8(_t(gpu, x)).cpu().numpy()
    want = K.encode(x)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


def test_dequant_f8_is_the_table(gpu):
    import torch
    from simplellminference_amd import ops
    codes = np.arange(256, dtype=np.uint8)
    got = ops.dequant_f8(_t(gpu, codes)).cpu().numpy()
    nan = (codes & 0x7F) == 0x7F
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), K.TABLE[~nan].view(np.uint32))
    got8 = ops.dequant_f8(_t(gpu, codes).view(torch.float8_e4m3fn)).cpu().numpy()
    assert np.array_equal(got8[~nan].view(np.uint32), got[~nan].view(np.uint32))


# ---------------------------------------------------------------- 2. the attention op against the oracle
MHA_SHAPES = [
    # position 0 and a masked first tile
    (64, 64, 4, 4, 1, 0), (64, 64, 4, 2, 0, 35), (64, 64, 4, 2, 1, 63),
    # one kv head with 8 query heads
    (300, 128, 8, 1, 0, 299),
    # the split cap (one kv head, 16 splits of 256 keys) and split / tile boundaries
    (4096, 128, 4, 1, 0, 4095), (4096, 128, 4, 1, 1, 255), (4096, 128, 32, 8, 1, 1024), (4096, 64, 16, 2, 0, 129),
    # the partial buffer's own split at hd 64 (256 keys: never a shorter split)
    (1024, 64, 16, 2, 1, 1023),
    # 4 tiles per wave: the ring is refilled, with waves of unequal live tiles
    (16384, 128, 32, 8, 1, 16383), (16384, 128, 32, 8, 0, 15683), (16384, 128, 32, 8, 1, 607)]


@functools.lru_cache(maxsize=None)
def _mha_case(T, hd, H, Hkv, pos):
    """q and an FP8 cache of random normal values (codes, and the decoded fp32 values the oracle reads)."""
    r = np.random.default_rng(T + pos)
    L, kv = 2, Hkv * hd
    q = r.standard_normal(H * hd).astype(np.float32)
    kq = K.encode(r.standard_normal((L, T, kv)).astype(np.float32))
    vq = K.encode(r.standard_normal((L, T, kv)).astype(np.float32))
    return q, kq, vq, K.decode(kq), K.decode(vq)


@pytest.mark.parametrize("T,hd,H,Hkv,layer,pos", MHA_SHAPES)
def test_mha_f8(gpu, oracle, T, hd, H, Hkv, layer, pos):
    import torch
    from simplellminference_amd import ops
    q, kq, vq, kf, vf = _mha_case(T, hd, H, Hkv, pos)
    want = oracle.mha(q, kf, vf, layer, pos, T, hd, H, Hkv)
    got = ops.mha(_t(gpu, q), _t(gpu, kq), _t(gpu, vq), layer, pos, T, hd, H, Hkv, kv_dtype="f8")
    _close(got.cpu().numpy(), want, rtol=1e-5, atol=2e-6)
    if T == 64:  # the same bytes as a float8_e4m3fn tensor
        got8 = ops.mha(_t(gpu, q), _t(gpu, kq).view(torch.float8_e4m3fn), _t(gpu, vq).view(torch.float8_e4m3fn), layer,
                       pos, T, hd, H, Hkv)
        assert torch.equal(got, got8)


def test_mha_f8_extreme_values_decode(gpu, oracle):
    """V rows of +-448 and +-2^-9 (the largest value and the smallest subnormal) where the softmax puts all its
    weight: k = 0 everywhere makes every key's weight 1 / (pos + 1) exactly, so the output is the mean of V."""
    from simplellminference_amd import ops
    T, hd, H, Hkv, pos = 64, 64, 4, 2, 3
    q = np.ones(H * hd, np.float32)
    kq = np.zeros((1, T, Hkv * hd), np.uint8)
    vq = np.zeros((1, T, Hkv * hd), np.uint8)
    vq[0, 0], vq[0, 1], vq[0, 2], vq[0, 3] = 0x7E, 0xFE, 0x01, 0x81  # 448, -448, 2^-9, -2^-9
    vq[0, 2, ::2] = 0x7E   # even columns: 448 - 448 + 448 - 2^-9
    vq[0, 0, 1::4] = 0x01  # some columns: 2^-9 - 448 + 2^-9 - 2^-9
    want = oracle.mha(q, K.decode(kq), K.decode(vq), 0, pos, T, hd, H, Hkv)
    assert np.unique(want).size >= 3
    got = ops.mha(_t(gpu, q), _t(gpu, kq), _t(gpu, vq), 0, pos, T, hd, H, Hkv, kv_dtype="f8").cpu().numpy()
    _close(got, want, rtol=1e-6, atol=0)
    # a subnormal alone survives (nothing flushes it): one live key holding +-2^-9
    vq1 = np.full((1, T, Hkv * hd), 0x01, np.uint8)
    vq1[0, :, 1::2] = 0x81
    got = ops.mha(_t(gpu, q), _t(gpu, kq), _t(gpu, vq1), 0, 0, T, hd, H, Hkv, kv_dtype="f8").cpu().numpy()
    assert np.array_equal(got, np.tile(np.array([2.0 ** -9, -2.0 ** -9], np.float32), H * hd // 2))
    # and K: q . k with k = +-448 / 2^-9 codes against the oracle
    r = np.random.default_rng(5)
    kq2 = r.choice(np.array([0x7E, 0xFE, 0x01, 0x81, 0x08, 0x38], np.uint8), (1, T, Hkv * hd))
    vq2 = K.encode(r.standard_normal((1, T, Hkv * hd)).astype(np.float32))
    q2 = (r.standard_normal(H * hd) * 1e-3).astype(np.float32)
    want = oracle.mha(q2, K.decode(kq2), K.decode(vq2), 0, 40, T, hd, H, Hkv)
    got = ops.mha(_t(gpu, q2), _t(gpu, kq2), _t(gpu, vq2), 0, 40, T, hd, H, Hkv, kv_dtype="f8").cpu().numpy()
    _close(got, want, rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("T,hd,H,Hkv,pos", [(4096, 128, 32, 8, 4095), (1024, 64, 16, 2, 700)])
def test_mha_f8_head_major_strides(gpu, oracle, T, hd, H, Hkv, pos):
    """The engine's layout [Hkv][T][hd] through sli_mha_strided, against the same oracle call."""
    from simplellminference_amd import ops
    q, kq, vq, kf, vf = _mha_case(T, hd, H, Hkv, pos)
    want = oracle.mha(q, kf, vf, 1, pos, T, hd, H, Hkv)
    hm = lambda c: np.ascontiguousarray(c[1].reshape(T, Hkv, hd).transpose(1, 0, 2))
    got = ops.mha_strided(_t(gpu, q), _t(gpu, hm(kq)), _t(gpu, hm(vq)), pos, T, hd, H, Hkv, hd, T * hd, kv_dtype="f8")
    _close(got.cpu().numpy(), want, rtol=1e-5, atol=2e-6)


# ---------------------------------------------------------------- 3. argument checks
def test_mha_f8_argument_checks(gpu):
    """The statuses of include/sli.h. Where the fp16 call refuses the same mistake (null pointers, head counts, head
    size, position, a short workspace) the FP8 call gives the same status; the alignment refusals are the FP8 cache's
    own (the fp16 cache has a register-staged kernel to fall back on, the FP8 cache has none)."""
    torch = gpu
    from simplellminference_amd import _lib
    L = _lib.load()
    T, hd, H, Hkv = 256, 64, 4, 2
    q = torch.zeros(H * 128 + 8, dtype=torch.float32, device="cuda")
    c8 = torch.zeros(2 * T * 8 * 128 + 64, dtype=torch.uint8, device="cuda")
    c16 = torch.zeros(2 * T * 8 * 128 + 64, dtype=torch.float16, device="cuda")
    out = torch.zeros(8 * 128, dtype=torch.float32, device="cuda")
    nws = L.sli_mha_workspace_bytes(T, 8, 128)
    ws = torch.zeros(nws // 4 + 1, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    F16, F8 = _lib.DT_F16, _lib.DT_F8E4M3
    ARG, SHAPE, RANGE = 1, 2, 3

    def mha(dt, c, qp=None, kp=None, vp=None, op=None, wp=None, pos=10, hd_=hd, H_=H, Hkv_=Hkv, nbytes=None):
        nb = L.sli_mha_workspace_bytes(T, H_, hd_) if nbytes is None else nbytes
        return L.sli_mha(p(q) if qp is None else qp, p(c) if kp is None else kp, p(c) if vp is None else vp, dt,
                         p(out) if op is None else op, 0, pos, T, hd_, H_, Hkv_, p(ws) if wp is None else wp, nb, None)

    same = {  # name -> (kwargs, status): both dtypes
        "ok": ({}, 0),
        "heads 3 per kv head": (dict(H_=6, Hkv_=2), SHAPE),
        "heads not a multiple": (dict(H_=5, Hkv_=2), SHAPE),
        "head_dim 32": (dict(hd_=32), SHAPE),
        "position past the cache": (dict(pos=T), RANGE),
        "workspace one byte short": (dict(nbytes=L.sli_mha_workspace_bytes(T, H, hd) - 1), ARG),
    }
    for name, (kw, want) in same.items():
        assert mha(F16, c16, **kw) == want, (name, "f16")
        assert mha(F8, c8, **kw) == want, (name, "f8")
    for name, kw in {"null q": dict(qp=ctypes.c_void_p(0)), "null k": dict(kp=ctypes.c_void_p(0)),
                     "null v": dict(vp=ctypes.c_void_p(0)), "null out": dict(op=ctypes.c_void_p(0)),
                     "null workspace": dict(wp=ctypes.c_void_p(0))}.items():
        assert mha(F16, c16, **kw) == ARG, (name, "f16")
        assert mha(F8, c8, **kw) == ARG, (name, "f8")
    # the FP8 cache's own: every DMA piece is 16 bytes
    assert mha(F8, c8, kp=p(c8, 8)) == ARG
    assert mha(F8, c8, vp=p(c8, 4)) == ARG
    assert mha(F8, c8, qp=p(q, 4)) == ARG

    def strided(ps, hs):
        return L.sli_mha_strided(p(q), p(c8), p(c8), F8, p(out), 10, T, hd, H, Hkv, ps, hs, p(ws), nws, None)

    assert strided(Hkv * hd, hd) == 0
    assert strided(Hkv * hd + 8, hd) == ARG   # row stride not a multiple of 16 bytes
    assert strided(Hkv * hd + 16, hd + 8) == ARG  # head stride
    assert strided(0, hd) == ARG
    assert L.sli_mha(p(q), p(c8), p(c8), _lib.DT_I8, p(out), 0, 10, T, hd, H, Hkv, p(ws), nws, None) == ARG
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. the model against the float64 reference
from tests.test_kv8_ref_cpu import PROMPTS, PROMPTS8  # noqa: E402  (the ragged prompts of test_gpu_batch.py)

_W = {}


def _weights(oracle, name, seed, w_dtype):
    from simplellminference_amd.model import preset
    key = (name, seed, w_dtype)
    if key not in _W:
        _W[key] = K.weights(oracle, preset(name), seed, w_dtype)  # shared, never modified
    return _W[key]


def _gpu_run(make, toks, n):
    """A teacher-forced run of a fresh model from make(): logits [B, n, V] and the K / V rows [B][L][which] -> [n, KV]
    (a TPGroup's shards concatenated by kv head)."""
    gm = make()
    B = len(toks)
    if B == 1 and not hasattr(gm, "ranks"):
        _, logits = gm.predict(toks[0], n, want_logits=True)
        logits = logits[None]
    else:
        _, logits = gm.predict_batch(toks, n, want_logits=True)
    ranks = getattr(gm, "ranks", [gm])
    for b in range(B):
        assert all(m.state(b)["error"] == 0 for m in ranks)
    L = ranks[0].config.num_hidden_layers
    rows = [[[np.concatenate([m.kv(l, which, n, seq=b) for m in ranks], axis=1) for which in (0, 1)] for l in range(L)]
            for b in range(B)]
    gm.close()
    return logits, rows


def _model_against_reference(oracle, name, w_dtype, seed, prompts, n, make, what):
    """make(kv_dtype) -> a fresh model. The f32-cache model measures the slack against the unrounded float64 run; the
    f8-cache model's rows are walked by the FP8 float64 reference (tests/kv8_ref.py Walk), then its logits compared."""
    from simplellminference_amd.model import preset
    cfg = preset(name)
    oc, W = _weights(oracle, name, seed, w_dtype)
    toks = [K.pad_prompt(p, n, cfg.vocab_size, b) for b, p in enumerate(prompts)]
    _, rows32 = _gpu_run(lambda: make("f32"), toks, n)
    logits8, rows8 = _gpu_run(lambda: make("f8"), toks, n)
    for b in range(len(toks)):
        rows64, _ = K.unrounded_rows(oc, W, toks[b])
        slack = K.slack_from(rows64, lambda l, p, which: rows32[b][l][which][p])
        codes = [[K.encode(r) for r in kv] for kv in rows8[b]]
        for kv in rows8[b]:  # what the cache returns is on the FP8 grid
            for r in kv:
                assert np.array_equal(K.decode(K.encode(r)), r)
        ref, w = K.walk_run(oc, W, toks[b], lambda l, p, which: codes[l][which][p], slack)
        K.check_flips(w, f"{what} seq {b}")
        K.check_logits(logits8[b], ref, f"{what} seq {b}")


@pytest.mark.parametrize("name,w_dtype,seed", [("tiny", "f16", 4), ("tiny", "i8", 4), ("tiny-gqa", "f16", 11),
                                               ("tiny-gqa", "i8", 11), ("tiny-gqa", "mxfp4", 1)])
def test_model_batch1(gpu, oracle, name, w_dtype, seed):
    from simplellminference_amd.model import LlamaModel, preset
    make = lambda kv: LlamaModel(config=preset(name), w_dtype=w_dtype, kv_dtype=kv, seed=seed).init()
    _model_against_reference(oracle, name, w_dtype, seed, PROMPTS[:1], 36, make, f"{name} {w_dtype} batch 1")


@pytest.mark.parametrize("w_dtype", ["f16", "i8"])
def test_model_batch4(gpu, oracle, w_dtype):
    from simplellminference_amd.model import LlamaModel, preset
    name, seed = "tiny-gqa", 11
    make = lambda kv: LlamaModel(config=preset(name), w_dtype=w_dtype, kv_dtype=kv, seed=seed, batch=4).init()
    _model_against_reference(oracle, name, w_dtype, seed, PROMPTS, 36, make, f"{name} {w_dtype} batch 4")


def test_model_h128_batch8(gpu, oracle):
    from simplellminference_amd.model import LlamaModel, preset
    name, seed = "small-h128-gqa", 3
    make = lambda kv: LlamaModel(config=preset(name), w_dtype="i8", kv_dtype=kv, seed=seed, batch=8).init()
    _model_against_reference(oracle, name, "i8", seed, PROMPTS8, 24, make, f"{name} i8 batch 8")


# ---------------------------------------------------------------- 5. step structure and bytes
def test_step_structure_and_bytes(gpu):
    from simplellminference_amd._lib import SliError
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    m8 = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f8", seed=0).init()
    m16 = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=0).init()
    assert m8.exec_mode() == "launches" and m8.fused_qkv_attn() == 0 and m8.prefill_path() == "decode"
    with pytest.raises(SliError) as e:
        m8.set_prefill("gemm")
    assert e.value.code == 7 and "cannot take the GEMM prefill" in str(e.value)
    with pytest.raises(SliError):
        m8.set_exec("persist")
    assert m8.exec_mode() == "launches"
    with pytest.raises(SliError) as e:
        LlamaModel(config=cfg, w_dtype="f32", kv_dtype="f8", seed=0).init()
    assert e.value.code == 1
    with pytest.raises(SliError):  # MXFP4 weights stay batch 1
        LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f8", seed=0, batch=2).init()
    (w8, k8), (w16, k16) = m8.step_bytes(), m16.step_bytes()
    assert w8 == w16 and k8 * 2 == k16 and k8 > 0
    m16.close()
    prompt = [1, 17, 42, 99, 7, 3]
    t1, l1 = m8.predict(prompt, 20, want_logits=True)
    m8.reset()
    t2, l2 = m8.predict_prefill(prompt, 20, want_logits=True)
    m8.close()
    assert np.array_equal(t1, t2)
    live = ~np.isnan(l2).any(axis=1)  # predict_prefill leaves the prompt's unused logits rows NaN
    assert live[len(prompt) - 1:].all()
    assert np.array_equal(l1[live].view(np.uint32), l2[live].view(np.uint32))


# ---------------------------------------------------------------- 6. cache I/O
@pytest.mark.parametrize("name,w_dtype,seed", [("tiny-gqa", "f16", 11), ("small-h128-gqa", "i8", 3)])
def test_cache_io(gpu, oracle, name, w_dtype, seed):
    """fill_kv_synthetic rounds through the shared rule (the f32-cache model's rows for the same seed, encoded and
    decoded, bit for bit), and a step at position `upto` over those rows matches the reference started from them."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset(name)
    upto, L = 20, cfg.num_hidden_layers
    m32 = LlamaModel(config=cfg, w_dtype=w_dtype, kv_dtype="f32", seed=seed).init()
    m8 = LlamaModel(config=cfg, w_dtype=w_dtype, kv_dtype="f8", seed=seed).init()
    for m in (m32, m8):
        m.fill_kv_synthetic(7, upto)
    cache32 = [np.stack([m32.kv(l, which, upto) for l in range(L)]) for which in (0, 1)]
    cache = [K.decode(K.encode(c)) for c in cache32]
    for which in (0, 1):
        for l in range(L):
            assert np.array_equal(m8.kv(l, which, upto).view(np.uint32), cache[which][l].view(np.uint32))
    assert np.abs(cache[0]).max() > 0 and not np.array_equal(cache[0], cache32[0])
    tok = 42
    rows = {}
    logits = {}
    for kv, m in (("f32", m32), ("f8", m8)):
        logits[kv] = m.forward(tok, upto)
        rows[kv] = [[m.kv(l, which, upto + 1)[upto] for which in (0, 1)] for l in range(L)]
    logits8 = logits["f8"]
    assert m8.state()["error"] == 0
    m32.close()
    m8.close()
    # the slack, as in part 4: the f32-cache model's new rows against the unrounded reference over the same
    # (unrounded synthetic) rows
    oc, W = _weights(oracle, name, seed, w_dtype)
    un = K.Model8(oc, W, rounding=False)
    un.kc[:, :upto], un.vc[:, :upto] = cache32
    un.forward(tok, upto)
    slack = K.slack_from([un.last_rows], lambda l, p, which: rows["f32"][l][which])
    codes = [[K.encode(r) for r in kv] for kv in rows["f8"]]
    ref, w = K.walk_run(oc, W, [tok], lambda l, p, which: codes[l][which], slack, start=upto, cache=cache)
    K.check_flips(w, f"{name} cache I/O")
    K.check_logits(logits8[None], ref, f"{name} cache I/O")


# ---------------------------------------------------------------- 7. tensor parallelism
def test_tp_group(gpu, oracle):
    from simplellminference_amd.model import TPGroup, preset
    name, seed = "tiny-h8", 4
    make = lambda kv: TPGroup(preset(name), 2, w_dtype="i8", kv_dtype=kv, seed=seed, batch=4).init()
    _model_against_reference(oracle, name, "i8", seed, PROMPTS, 36, make, f"{name} i8 TP-2 group batch 4")


# (The two-process fused_wg run is left out: tests/test_gpu_tp.py::_oneshot_rank builds its model with kv_dtype
# "f16" and takes no cache dtype, and that file stays as it is.)


# ---------------------------------------------------------------- 8. determinism
def test_determinism(gpu):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("small-h128-gqa")
    toks = [K.pad_prompt(p, 24, cfg.vocab_size, b) for b, p in enumerate(PROMPTS)]
    runs = []
    for _ in range(2):
        logits, rows = _gpu_run(lambda: LlamaModel(config=cfg, w_dtype="i8", kv_dtype="f8", seed=3, batch=4).init(),
                                toks, 24)
        runs.append((logits, np.array(rows)))
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    assert np.array_equal(K.encode(runs[0][1]), K.encode(runs[1][1]))
