"""The model path of the block-scaled MFMA prefill: LlamaModel.set_prefill("gemm-mx8") (SLI_PREFILL_GEMM_MX8), on the tiny
presets, whose projection depths (256, 768) lie on 128."""
import numpy as np
import pytest

from simplellminference_amd.tp import KINDS

pytestmark = pytest.mark.gpu


def _prompt(n, vocab, seed=3):
    return [int(t) for t in np.random.default_rng(seed + n).integers(0, vocab, n)]


def _model(w="mxfp4", kv="f16", name="tiny-gqa", seed=7, **over):
    from simplellminference_amd.model import LlamaModel, preset
    return LlamaModel(config=preset(name, **over), w_dtype=w, kv_dtype=kv, seed=seed).init()


def _run(m, prompt, mode):
    m.reset()
    m.set_prefill(mode)
    assert m.prefill_path() == "mfma"
    _, logits = m.predict_prefill(prompt, len(prompt) + 1, want_logits=True)
    L = m.config.num_hidden_layers
    return np.stack([m.kv(l, w, len(prompt) - 1) for l in range(L) for w in (0, 1)]), logits[len(prompt) - 1]


def test_refusals(gpu):
    from simplellminference_amd._lib import SliError
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    made = [_model(w="f16"), _model(w="i8"), _model(w="f32", kv="f32"), _model(kv="f32"),
            _model(intermediate_size=704, max_length=160),  # 704 = 5.5 * 128
            LlamaModel(config=preset("tiny-gqa"), w_dtype="mxfp4", kv_dtype="f16", seed=7, batch=2, mx_batch=True).init(),
            TPGroup(preset("tiny-h8"), tp_size=2, w_dtype="mxfp4", kv_dtype="f16", seed=5).init()]
    for m in made:
        with pytest.raises(SliError) as e:
            m.set_prefill("gemm-mx8")
        assert e.value.code == 7, e.value  # SLI_ERR_STATE
        m.close()
    m = _model(kv="f8")  # accepted, and a prompt runs through the FP8-cache epilogue and attention behind it
    rows, logits = _run(m, _prompt(40, m.config.vocab_size), "gemm-mx8")
    m.close()
    assert np.isfinite(rows).all() and np.isfinite(logits).all() and np.abs(rows).max() > 0


def test_layer0_rows_equal_the_op_chain(gpu):
    """Weights through set_weight, 40 tokens (39 rows, a 64-row chunk): layer 0's rows equal the op-level chain."""
    torch = gpu
    from simplellminference_amd import ops
    m = _model()
    c = m.config
    hq, hkv, hd, D, T = c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.hidden_size, c.max_length
    r = np.random.default_rng(11)
    emb = r.standard_normal((c.vocab_size, D)).astype(np.float32)
    norm = r.uniform(0.5, 1.5, D).astype(np.float32)
    wq, wk, wv = ((r.standard_normal((h * hd, D)) / np.sqrt(D)).astype(np.float32) for h in (hq, hkv, hkv))
    for kind, idx, t in (("emb", 0, emb), ("norm", 0, norm), ("wq", 0, wq), ("wk", 0, wk), ("wv", 0, wv)):
        m.set_weight(KINDS[kind], idx, t)
    prompt = _prompt(40, c.vocab_size)
    m.set_prefill("gemm-mx8")
    m.prefill(prompt)
    got = [m.kv(0, w, 39) for w in (0, 1)]
    m.close()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    table = ops.dequant_mxfp4(*ops.quant_mxfp4(dev(emb)))
    rows = prompt[:39] + [prompt[38]] * 25  # a group's padding rows repeat its last valid token
    x = table[torch.tensor(rows, device="cuda")].contiguous()
    ac, a_s = ops.prefill_norm_quant_mx8(x, dev(norm), c.rms_norm_eps)
    data, ws = ops.quant_mxfp4(dev(np.concatenate([wq, wk, wv])))
    sin_t, cos_t = ops.rope_cache(hd, T, c.rope_theta)
    q = torch.empty(64, hq * hd, device="cuda")
    kc = torch.zeros(hkv, T, hd, device="cuda", dtype=torch.float16)
    vc = torch.zeros_like(kc)
    ops.prefill_gemm_qkv_mx8(data, ws, ac, a_s, q, kc, vc, sin_t, cos_t, hq, hkv, hd, 0, 39)
    for g, cache in zip(got, (kc, vc)):
        ref = cache[:, :39].permute(1, 0, 2).reshape(39, hkv * hd).float().cpu().numpy()
        assert np.array_equal(g, ref), int((g != ref).sum())


def test_split_equals_whole(gpu):
    """30 tokens at once against 20 and extend_one from position 19 (32-row chunks all): bit for bit."""
    m = _model()
    prompt = _prompt(30, m.config.vocab_size)
    whole = _run(m, prompt, "gemm-mx8")
    m.reset()
    m.prefill(prompt[:20])
    m.extend_one(prompt[19:], start=19)
    m.step()
    m.sync()
    L = m.config.num_hidden_layers
    rows = np.stack([m.kv(l, w, 29) for l in range(L) for w in (0, 1)])
    logits = m.logits()[0]
    m.close()
    assert np.array_equal(rows, whole[0]) and np.array_equal(np.asarray(logits).ravel(), whole[1].ravel())


def test_close_to_gemm_and_switching(gpu):
    """(d) ||mx8 - gemm|| <= ||gemm - f16|| on the first-step logits: e4m3 activations (3 mantissa bits) add less error
    than the FP4 weights (1 bit) already cost; (e) gemm -> gemm-mx8 -> gemm repeats the first gemm result bit for bit."""
    m = _model()
    prompt = _prompt(40, m.config.vocab_size)
    g1, x8, g2 = (_run(m, prompt, mode) for mode in ("gemm", "gemm-mx8", "gemm"))
    m.close()
    h = _model(w="f16")
    f16 = _run(h, prompt, "gemm")
    h.close()
    assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1])
    d_mx8, d_w = float(np.linalg.norm(x8[1] - g1[1])), float(np.linalg.norm(g1[1] - f16[1]))
    assert d_mx8 <= d_w, (d_mx8, d_w)
