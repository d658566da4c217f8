"""The batch-1 GEMVs' hot argument block and the host-side unit partition (gemv.h GemvPart / udiv / epi_prepare):
tiny shapes that take each branch of the GEMV index math that moved from the kernels to the launch sites, and the
decode kernels whose arguments the build now preloads (attention, embedding, key reduce; their sources are
unchanged). Each case is held to the C oracle at the bars tests/test_gpu_ops.py and tests/test_gpu_model.py apply to
the same ops (their `_close` with the same rtol / atol, which those files keep inline; the model step's 1e-3 on
logits and the same argmax), and run twice for bit-identical results.

The chip has 256 workgroups x 16 waves = 4096 GEMV waves; op-level GEMVs run two-row units (R = 2).
"""
import numpy as np
import pytest

from tests.test_gpu_ops import _close, _rng, _t

pytestmark = pytest.mark.gpu

# rows, cols (fp16: 8 columns per 16-byte vector, int8: 16)
GEMV_SHAPES = [
    (1, 4096),      # one unit, one workgroup, every wave but the column parts' idle
    (2, 4096),      # one full unit
    (96, 4096),     # a column-split shard shape: 48 units x 8 parts, fewer items than waves
    (40, 256),      # fewer units than waves and fewer chunks than parts
    (8198, 256),    # 4099 units on 4096 waves: not divisible, waves of 1 and 2 units, workgroups of 16 and 17
    (8200, 2736),   # a masked last chunk (342 fp16 / 171 int8 vectors), unsplit
    (600, 2744),    # 343 fp16 vectors, column split with a masked last part
]


@pytest.mark.parametrize("rows,cols", GEMV_SHAPES)
def test_gemv_f16_partition(gpu, oracle, rows, cols):
    torch = gpu
    from simplellminference_amd import ops
    r = _rng(rows * 3 + cols)
    x = r.standard_normal(cols).astype(np.float32)
    w16 = (r.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float16)
    want = oracle.matmul(x, w16.astype(np.float32))
    tx, tw = _t(torch, x), _t(torch, w16)
    got = ops.matmul(tx, tw)
    again = ops.matmul(tx, tw)
    assert torch.equal(got, again)
    _close(got.cpu().numpy(), want, rtol=1e-4, atol=1e-4)  # test_gpu_ops.test_matmul_f16_weights


@pytest.mark.parametrize("rows,cols", [s for s in GEMV_SHAPES if s[1] % 16 == 0])
def test_gemv_i8_partition(gpu, oracle, rows, cols):
    torch = gpu
    from simplellminference_amd import ops
    r = _rng(5 + rows + cols)
    x = r.standard_normal(cols).astype(np.float32)
    w = (r.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float32)
    q = np.empty((rows, cols), np.int8)
    s = np.empty(rows, np.float32)
    for i in range(rows):
        q[i], s[i] = oracle.quant_row_i8(w[i])
    want = oracle.matmul(x, q.astype(np.float32) * s[:, None])
    tx, tq, ts = _t(torch, x), _t(torch, q), _t(torch, s)
    got = ops.matmul(tx, tq, row_scale=ts)
    again = ops.matmul(tx, tq, row_scale=ts)
    assert torch.equal(got, again)
    _close(got.cpu().numpy(), want, rtol=1e-4, atol=1e-4)  # test_gpu_ops.test_matmul_i8_weights


# attn_partial_kernel (an fp32 cache runs it at every group size): hd 128 splits the context every 128 positions,
# hd 64 every 256, so the positions sit on, before and after a split boundary of both
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2)])
@pytest.mark.parametrize("pos", [0, 127, 128, 255, 256, 257])
def test_attn_partial_positions(gpu, oracle, hd, H, Hkv, pos):
    torch = gpu
    from simplellminference_amd import ops
    T, L, layer = 512, 2, 1
    r = _rng(hd + 7 * H + Hkv + pos)
    q = r.standard_normal(H * hd).astype(np.float32)
    kc = r.standard_normal((L, T, Hkv * hd)).astype(np.float32)
    vc = r.standard_normal((L, T, Hkv * hd)).astype(np.float32)
    want = oracle.mha(q, kc, vc, layer, pos, T, hd, H, Hkv)
    tq, tk, tv = _t(torch, q), _t(torch, kc), _t(torch, vc)
    got = ops.mha(tq, tk, tv, layer, pos, T, hd, H, Hkv)
    again = ops.mha(tq, tk, tv, layer, pos, T, hd, H, Hkv)
    assert torch.equal(got, again)
    _close(got.cpu().numpy(), want, rtol=1e-5, atol=2e-6)  # test_gpu_ops.test_mha


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_embedding_first_and_last_token(gpu, oracle, dtype):
    torch = gpu
    from simplellminference_amd import ops
    tab = _rng(13).standard_normal((512, 256)).astype(np.float32)
    if dtype == "f16":
        tab = tab.astype(np.float16)
    tt = _t(torch, tab)
    for tok in (0, 511):
        want = oracle.embedding(tok, tab.astype(np.float32))
        assert np.array_equal(ops.embedding(tok, tt).cpu().numpy(), want)
        dev = torch.tensor([tok], dtype=torch.int32, device="cuda")  # the device token: the kernel's first load
        assert np.array_equal(ops.embedding(dev, tt).cpu().numpy(), want)


# The engine's step: the R = 2 epilogues (RoPE pairs + K/V write, SwiGLU, logits + argmax keys), the merge-staged
# K-split wo, the fp16-cache attention with its splits merged by wo, the embedding and the key reduce. One layer
# at Llama-2-7B's width (the K-split wo and its summing consumers need D = 4096), a short FFN and an odd vocabulary
# (the last logits unit holds one row). The oracle and the model are built once and stepped in the same order.
def _step_model(oracle, name, **over):
    from simplellminference_amd.model import preset
    cfg = preset(name, **over)
    ocfg = oracle.Config(cfg.vocab_size, cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads,
                         cfg.head_dim, cfg.intermediate_size, cfg.num_hidden_layers, cfg.max_length,
                         cfg.rms_norm_eps, cfg.rope_theta)
    return cfg, ocfg


def _check_steps(oracle, cfg, ocfg, w, steps, fill):
    from simplellminference_amd.model import LlamaModel
    wmode = {"f16": oracle.W_F16, "i8": oracle.W_I8}[w]
    om = oracle.Model(ocfg, seed=4, wmode=wmode, kv_f16=True)
    gm = LlamaModel(config=cfg, w_dtype=w, kv_dtype="f16", seed=4).init()
    if fill:
        om.fill_kv_synthetic(7, fill)
        gm.fill_kv_synthetic(7, fill)
    for tok, pos in steps:
        want = om.forward(tok, pos)
        got = gm.forward(tok, pos)
        again = gm.forward(tok, pos)
        assert np.array_equal(got, again), (tok, pos)
        err = float(np.abs(got - want).max())
        print(f"{w} token {tok} pos {pos}: max|dlogit| {err:.3e}")
        assert err <= 1e-3, (tok, pos, err)  # test_gpu_model's bar
        assert int(np.argmax(got)) == int(np.argmax(want)), (tok, pos)
        st = gm.state()
        assert st["error"] == 0 and st["last_argmax"] == int(np.argmax(got)), (tok, pos, st)  # the key reduce
    gm.close()
    om.close()


# head_dim 128, MHA and GQA-2, ctx 2048 (splits of 256 positions): 1, 3 and 8 live splits; the split boundary;
# the first and the last token id (the embedding's rows); pos 0 and pos > 0 for RoPE
@pytest.mark.parametrize("w", ["f16", "i8"])
@pytest.mark.parametrize("hkv", [32, 16])
def test_step_hd128(gpu, oracle, w, hkv):
    cfg, ocfg = _step_model(oracle, "llama2-7b", num_hidden_layers=1, intermediate_size=1376, vocab_size=1001,
                            num_key_value_heads=hkv, kv_hidden_size=hkv * 128)
    steps = [(0, 0), (1000, 255), (17, 256), (5, 257), (3, 600), (1000, 2047)]
    _check_steps(oracle, cfg, ocfg, w, steps, 2047)


# head_dim 64 (RoPE pairs 32 apart; the tiny shapes run the column-split GEMVs and the unsplit wo)
@pytest.mark.parametrize("name", ["tiny", "tiny-gqa"])
def test_step_hd64(gpu, oracle, name):
    cfg, ocfg = _step_model(oracle, name)
    steps = [(0, 0), (511, 35), (9, 63)]
    _check_steps(oracle, cfg, ocfg, "f16", steps, 63)


# The key reduce with the winning key at the first and at the last token id: the first slot of the first LM-head
# workgroup's key and the last slot of the last one's (vocab 1001: id 1000 is the one-row last logits unit). The
# argmax is forced there by scaling that row of the tied embedding / LM head by a signed power of two (exact in
# fp16, and in int8 through the row scale) on the oracle's weights, which the model is then given; the input token
# is another row, so only that logit moves.
@pytest.mark.parametrize("w", ["f16", "i8"])
@pytest.mark.parametrize("row", ["first", "last"])
def test_keyreduce_first_and_last_token(gpu, oracle, w, row):
    from simplellminference_amd.model import LlamaModel
    from simplellminference_amd.tp import KINDS
    cfg, ocfg = _step_model(oracle, "llama2-7b", num_hidden_layers=1, intermediate_size=1376, vocab_size=1001)
    r = 0 if row == "first" else cfg.vocab_size - 1
    tok, pos = 17, 3
    om = oracle.Model(ocfg, seed=4, wmode={"f16": oracle.W_F16, "i8": oracle.W_I8}[w], kv_f16=True)
    om.fill_kv_synthetic(7, pos)
    base = om.forward(tok, pos)
    k = 2.0 ** np.ceil(np.log2(2.0 * np.abs(base).max() / abs(base[r])))  # |logit r| becomes >= 2 max|logit|
    emb = om.weight(oracle.T_EMB)  # a view of the oracle's own (already rounded / dequantised) table
    emb[r] *= np.float32(k if base[r] > 0 else -k)
    assert np.abs(emb[r]).max() < 6.0e4  # still finite in fp16
    want = om.forward(tok, pos)
    assert int(np.argmax(want)) == r
    gm = LlamaModel(config=cfg, w_dtype=w, kv_dtype="f16", seed=4).init()
    gm.set_weight(KINDS["emb"], 0, emb)
    gm.fill_kv_synthetic(7, pos)
    got = gm.forward(tok, pos)
    st = gm.state()
    again = gm.forward(tok, pos)
    assert np.array_equal(got, again) and gm.state()["last_argmax"] == st["last_argmax"]
    err = float(np.abs(got - want).max())
    print(f"{w} forced id {r}: logit {want[r]:.3f}, max|dlogit| {err:.3e}")
    # test_gpu_model's 1e-3 bar is for O(1) logits; the forced logit is held to the same bar relative to its size
    assert np.abs(np.delete(got, r) - np.delete(want, r)).max() <= 1e-3
    assert abs(got[r] - want[r]) <= 1e-3 * max(1.0, abs(want[r]))
    assert int(np.argmax(got)) == r and st["error"] == 0 and st["last_argmax"] == r, st
    gm.close()
    om.close()
