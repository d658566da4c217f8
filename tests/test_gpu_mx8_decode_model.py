"""The model path of the block-scaled batched decode step: LlamaModel.set_decode("mx8") (SLI_DECODE_MX8) on the tiny
presets (projection depths 256 and 768: multiples of 128), batch 3."""
import numpy as np
import pytest

from simplellminference_amd.tp import KINDS

pytestmark = pytest.mark.gpu
TOKENS, POSITIONS = [5, 77, 130], [0, 3, 6]


def _model(w="mxfp4", kv="f16", batch=3, name="tiny-gqa", **over):
    from simplellminference_amd.model import LlamaModel, preset
    return LlamaModel(config=preset(name, **over), w_dtype=w, kv_dtype=kv, seed=7, batch=batch,
                      mx_batch=w == "mxfp4" and batch > 1).init()


def _first_step(m):
    m.reset()
    return m.forward_batch(TOKENS, [0, 0, 0]).copy()


@pytest.mark.parametrize("kv", ["f16", "f8"])
def test_mode_runs_and_switches_back(gpu, kv):
    """12 greedy steps behind ragged prompts; ||mx8 - auto|| < ||auto - fp16 weights|| on the first step's logits (e4m3
    activations cost less than the FP4 weights already do: tests/test_gpu_mx8_model.py's inequality); back under "auto"
    the step repeats its earlier logits bit for bit, which holds only if the weight images were re-laid."""
    m = _model(kv=kv)
    V = m.config.vocab_size
    prompts = [[int(t) for t in np.random.default_rng(n).integers(0, V, n)] for n in (3, 7, 5)]
    a1 = _first_step(m)
    assert m.decode_path() == "auto" and m.set_decode("mx8").decode_path() == "mx8"
    x8 = _first_step(m)
    m.reset()
    toks, logits = m.predict_batch(prompts, 7 + 12, want_logits=True)
    assert np.isfinite(logits).all() and (toks >= 0).all() and (toks < V).all()
    m.set_sampling(temperature=0.8, top_k=20, seed=3)  # the sampler launch joins the step under the mode
    m.reset()
    m.forward_batch(TOKENS, [0, 0, 0])
    assert all(0 <= m.sampled(b) < V for b in range(3))
    m.set_sampling(None)
    out = m.generate([dict(prompt=p, max_new_tokens=4) for p in prompts])
    assert all(len(o["tokens"]) == 4 for o in out)
    m.set_sampling(None)
    assert m.set_decode("auto").decode_path() == "auto"
    a2 = _first_step(m)
    m.close()
    h = _model(w="f16", kv=kv)
    f16 = _first_step(h)
    h.close()
    assert np.array_equal(a1, a2)
    d8, dw = float(np.linalg.norm(x8 - a1)), float(np.linalg.norm(a1 - f16))
    assert 0 < d8 < dw, (d8, dw)


def test_layer0_qkv_equals_the_op(gpu):
    """Layer 0's K / V rows of one model step equal ops.batch_gemm_qkv_mx8 on the same inputs, bit for bit."""
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
    m.set_decode("mx8")
    m.forward_batch(TOKENS, POSITIONS)
    got = [[m.kv(0, w, p + 1, seq=b)[p] for b, p in enumerate(POSITIONS)] for w in (0, 1)]
    m.close()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x = ops.dequant_mxfp4(*ops.quant_mxfp4(dev(emb)))[torch.tensor(TOKENS, device="cuda")].contiguous()
    data, ws = ops.quant_mxfp4(dev(np.concatenate([wq, wk, wv])))
    sin_t, cos_t = ops.rope_cache(hd, T, c.rope_theta)
    q = torch.empty(8, hq * hd, device="cuda")
    kc = torch.zeros(3, hkv, T, hd, device="cuda", dtype=torch.float16)
    vc = torch.zeros_like(kc)
    ops.batch_gemm_qkv_mx8(x, dev(norm), c.rms_norm_eps, data, q, kc, vc, dev(np.asarray(POSITIONS, np.int32)), sin_t, cos_t,
                           hq, hkv, hd, tiled=True, scales=ws)
    for g, cache in zip(got, (kc, vc)):
        for b, p in enumerate(POSITIONS):
            ref = cache[b, :, p].reshape(hkv * hd).float().cpu().numpy()
            assert np.array_equal(np.asarray(g[b]).ravel(), ref), (b, int((np.asarray(g[b]).ravel() != ref).sum()))


def test_refusals(gpu):
    from simplellminference_amd._lib import SliError
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    persist = LlamaModel(config=preset("small-h128"), w_dtype="f16", kv_dtype="f16", seed=1).init().set_exec("persist")
    group = TPGroup(preset("tiny-h8"), tp_size=2, w_dtype="mxfp4", kv_dtype="f16", seed=5, batch=2, mx_batch=True).init()
    cases = [(_model(w="f16"), "MXFP4 weights"), (_model(batch=1), "batch 1"), (group.ranks[0], "in-process group"),
             (_model(intermediate_size=736, max_length=160), "multiples of 128"),  # 736 = 23 * 32
             (persist, "persistent layers")]
    for m, why in cases:
        with pytest.raises(SliError) as e:
            m.set_decode("mx8")
        assert e.value.code == 7 and why in str(e.value), e.value  # SLI_ERR_STATE
        assert m.decode_path() == "auto"
    with pytest.raises(SliError) as e:
        cases[0][0].set_decode("fp8")
    assert e.value.code == 1, e.value  # SLI_ERR_ARG: an unknown mode
    for m, _ in cases[:2] + cases[3:]:  # (the group's rank closes with its group)
        m.close()
    group.close()
