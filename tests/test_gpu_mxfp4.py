"""MXFP4 weights on the device: the quantiser against the numpy rule (tests/mxfp4_ref.py) bit for bit, the GEMV
against the C oracle on the rule's dequantised weights, and the model path against an eager oracle whose weights
were overwritten with that dequantisation."""
import numpy as np
import pytest

from tests import mxfp4_ref as mx

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float32).eps


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _weights(rows, cols, seed):
    """Gaussian rows / sqrt(cols) with the crafted corner blocks of mx.crafted() over the first rows."""
    r = np.random.default_rng(seed)
    w = (r.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float32)
    n = min(rows, 4)
    w[:n] = mx.crafted(n, cols, seed + 1)
    return w


# ---------------------------------------------------------------- 1. quantiser, bit exact
@pytest.mark.parametrize("rows,cols", [(4, 64), (7, 4096), (3, 11008)])
def test_quantiser_bit_exact(gpu, rows, cols):
    torch = gpu
    from simplellminference_amd import ops
    w = mx.crafted(rows, cols, seed=rows + cols)
    if rows > 4:
        w[4:] = (np.random.default_rng(1).standard_normal((rows - 4, cols)) / 64).astype(np.float32)
    codes, scales = mx.quantize(w)
    assert cols < 4096 or len(np.unique(scales)) > 8  # the crafted rows spread the block maxima
    data, sc = ops.quant_mxfp4(_t(torch, w))
    got_codes = mx.unpack(data.cpu().numpy())
    assert np.array_equal(sc.cpu().numpy(), scales)
    assert mx.same_codes(got_codes, codes), np.argwhere(got_codes != codes)[:8]
    deq = ops.dequant_mxfp4(data, sc).cpu().numpy()
    want = mx.dequantize(codes, scales)
    assert np.array_equal(deq, want)
    # the public layout is the helper's pack: the helper's bytes dequantise to the same values on the device
    deq2 = ops.dequant_mxfp4(_t(torch, mx.pack(codes)), _t(torch, scales)).cpu().numpy()
    assert np.array_equal(deq2, want) and np.array_equal(np.signbit(deq2), np.signbit(want))


def test_quantiser_refuses_bad_shapes(gpu):
    torch = gpu
    from simplellminference_amd import ops
    from simplellminference_amd._lib import SliError
    with pytest.raises(SliError):
        ops.quant_mxfp4(torch.zeros(5, 48, device="cuda"))
    with pytest.raises(SliError):
        ops.mxfp4_bytes(5, 48)
    x = torch.zeros(64, device="cuda")
    with pytest.raises(SliError):  # sli_matmul keeps rejecting dtype 3
        from simplellminference_amd._lib import call
        from simplellminference_amd.ops import _p, _s
        call("sli_matmul", _p(x), _p(x), 3, None, _p(x), 1, 64, 1.0, _s())


# ---------------------------------------------------------------- 2. GEMV
def _gemv_case(torch, oracle, w, x, scale=1.0):
    from simplellminference_amd import ops
    rows, cols = w.shape
    codes, scales = mx.quantize(w)
    deq = mx.dequantize(codes, scales)
    want = oracle.matmul(x, deq) * np.float32(scale)
    got = ops.matmul_mxfp4(_t(torch, x), _t(torch, mx.pack(codes)), _t(torch, scales), scale=scale).cpu().numpy()
    # test_matmul_f32's bound for a re-ordered fp32 sum (products of dequantised weights are exact to the same
    # degree), times |scale|
    bound = 4 * EPS * np.sqrt(cols) * (np.abs(deq) @ np.abs(x)) * abs(scale)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(err <= bound + 1e-30), (err.max(), (err - bound).max())
    return scales


# (8, 32): one vector per row, 63 lanes masked; (5, 96): odd rows, half a unit; (22, 11008): 344 vectors, a masked
# remainder chunk; (256 / 1000, 4096): fewer units than waves, the column-split path
@pytest.mark.parametrize("rows,cols", [(8, 32), (5, 96), (64, 4096), (22, 11008), (3, 14336), (256, 4096),
                                       (1000, 4096)])
def test_matmul_mxfp4(gpu, oracle, rows, cols):
    r = np.random.default_rng(rows * 3 + cols)
    x = r.standard_normal(cols).astype(np.float32)
    w = (r.standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float32)
    _gemv_case(gpu, oracle, w, x)


@pytest.mark.parametrize("rows,cols,scale", [(7, 4096, 1.0), (22, 11008, -0.375)])
def test_matmul_mxfp4_wide_range_and_scale(gpu, oracle, rows, cols, scale):
    r = np.random.default_rng(11)
    x = r.standard_normal(cols).astype(np.float32)
    w = _weights(rows, cols, seed=5)
    scales = _gemv_case(gpu, oracle, w, x, scale=scale)
    assert len(np.unique(scales)) > 2


def test_matmul_mxfp4_table_decode(gpu):
    """x = e_j for every j < 64: y[r] is element j of row r, exactly. Row r holds code (r + j) % 16 at column j, so
    every code meets both nibbles of a byte; the two blocks carry different scale bytes."""
    torch = gpu
    from simplellminference_amd import ops
    rows, cols = 16, 64
    codes = ((np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 16).astype(np.uint8)
    scales = np.stack([np.full(rows, 127 + 3, np.uint8), np.arange(rows).astype(np.uint8) + 100], axis=1)
    want = mx.dequantize(codes, scales)
    data, sc = _t(torch, mx.pack(codes)), _t(torch, scales)
    for j in range(cols):
        x = np.zeros(cols, np.float32)
        x[j] = 1.0
        got = ops.matmul_mxfp4(_t(torch, x), data, sc).cpu().numpy()
        assert np.array_equal(got, want[:, j]), (j, got, want[:, j])


# ---------------------------------------------------------------- model level
PROMPT = [1, 5, 9]
STEPS = 36
MATS = ("T_WQ", "T_WK", "T_WV", "T_WO", "T_UP", "T_GATE", "T_DOWN")


def _ocfg(oracle, cfg):
    return oracle.Config(cfg.vocab_size, cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads,
                         cfg.head_dim, cfg.intermediate_size, cfg.num_hidden_layers, cfg.max_length,
                         cfg.rms_norm_eps, cfg.rope_theta)


def mx_oracle(oracle, cfg, seed, kv_f16=True):
    """An eager fp32 oracle whose embedding and seven matrices per layer were overwritten in place with the rule's
    dequantisation (Model.weight() is a writable view); the LM head is tied to the embedding."""
    om = oracle.Model(_ocfg(oracle, cfg), seed=seed, wmode=oracle.W_F32, kv_f16=kv_f16)
    t = om.weight(oracle.T_EMB)
    t[...] = mx.quant_dequant(t)
    for l in range(cfg.num_hidden_layers):
        for name in MATS:
            w = om.weight(getattr(oracle, name), l)
            w[...] = mx.quant_dequant(w)
    return om


def min_top2_gap(logits):
    s = np.sort(logits, axis=-1)
    return float((s[..., -1] - s[..., -2]).min())


_REF = {}


def _tiny_ref(oracle, name, seed, kv):
    """Oracle tokens and logits of the parity run, computed once per (preset, seed, kv) and shared."""
    key = (name, seed, kv)
    if key not in _REF:
        from simplellminference_amd.model import preset
        om = mx_oracle(oracle, preset(name), seed, kv_f16=(kv == "f16"))
        _REF[key] = om.predict(PROMPT, STEPS)
        om.close()
    return _REF[key]


# Seeds chosen with the oracle alone: its smallest top-2 logit gap over the run is 1.6e-2 (tiny, seed 4) and 1.0e-2
# (tiny-gqa, seed 1), so a 1e-3 logit difference cannot flip a token (seeds 0 and 2 have gaps of 2e-4).
@pytest.mark.parametrize("name,seed,kv", [("tiny", 4, "f16"), ("tiny-gqa", 1, "f16"), ("tiny-gqa", 1, "f32")])
def test_model_parity(gpu, oracle, name, seed, kv):
    from simplellminference_amd.model import LlamaModel, preset
    otok, olog = _tiny_ref(oracle, name, seed, kv)
    gm = LlamaModel(config=preset(name), w_dtype="mxfp4", kv_dtype=kv, seed=seed).init()
    gtok, glog = gm.predict(PROMPT, STEPS, want_logits=True)
    gm.close()
    err = float(np.abs(glog - olog).max())
    print(f"{name} seed {seed} kv {kv}: max|dlogit| {err:.3e}, oracle min top-2 gap {min_top2_gap(olog):.3e}")
    assert np.array_equal(gtok, otok), (gtok, otok)
    assert err <= 1e-3, err


# ---------------------------------------------------------------- 4. placement and readback
def test_placement_and_readback(gpu, oracle, tmp_path):
    """Synthetic init, set_weight and the flat-file loader all quantise through the same rule: every matrix reads
    back as the helper's dequantisation of the oracle's fp32 weights, and the three models give bitwise the same
    logits. The norm vectors are not MXFP4 and are the one thing the device's synthetic generator does not
    reproduce to the bit (its 1 + c v differs from the host's in the last place for a few elements of each vector,
    for every weight type), so all three models are given the synthetic model's norms before they are compared."""
    from simplellminference_amd.model import LlamaModel, preset
    from simplellminference_amd.tp import KINDS
    cfg = preset("tiny-gqa")
    om = oracle.Model(_ocfg(oracle, cfg), seed=1, wmode=oracle.W_F32, kv_f16=True)  # the fp32 weights, as generated
    gm = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=1).init()
    sm = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=99).init()  # other weights, then overwritten
    emb = om.weight(oracle.T_EMB)
    assert np.array_equal(gm.weight_shard(KINDS["emb"]), mx.quant_dequant(emb))
    sm.set_weight(KINDS["emb"], 0, emb)
    for i in range(2 * cfg.num_hidden_layers + 1):
        n = om.weight(oracle.T_NORM, i)
        got_n = gm.weight_shard(KINDS["norm"], i)
        np.testing.assert_allclose(got_n, n, rtol=2e-7, atol=0)  # norms stay fp32 (see the docstring)
        sm.set_weight(KINDS["norm"], i, got_n)
    names = {"T_WQ": "wq", "T_WK": "wk", "T_WV": "wv", "T_WO": "wo", "T_UP": "up", "T_GATE": "gate", "T_DOWN": "down"}
    for l in range(cfg.num_hidden_layers):
        for oname, kname in names.items():
            w = om.weight(getattr(oracle, oname), l)
            assert np.array_equal(gm.weight_shard(KINDS[kname], l), mx.quant_dequant(w)), (kname, l)
            sm.set_weight(KINDS[kname], l, w)
    path = str(tmp_path / "w.bin")
    om.write_flat(path)
    fm = LlamaModel(model_path=path, config=cfg, w_dtype="mxfp4", kv_dtype="f16").init()
    for i in range(2 * cfg.num_hidden_layers + 1):
        fm.set_weight(KINDS["norm"], i, gm.weight_shard(KINDS["norm"], i))
    for kname in ("emb", "wq", "wo", "down"):  # the loader placed the same quantised matrices
        assert np.array_equal(fm.weight_shard(KINDS[kname], 0), gm.weight_shard(KINDS[kname], 0)), kname
    a_t, a_l = gm.predict(PROMPT, 12, want_logits=True)
    for other in (sm, fm):
        b_t, b_l = other.predict(PROMPT, 12, want_logits=True)
        assert np.array_equal(a_t, b_t)
        assert np.array_equal(a_l, b_l)  # bitwise: the same quantised weights through the same step
    for m_ in (gm, sm, fm):
        m_.close()
    om.close()


# ---------------------------------------------------------------- 5. 7B layer shapes
def test_llama7b_layer_shapes(gpu, oracle):
    """Llama-2-7B row shapes (D 4096, I 11008, 32 heads) at ctx 2048, one layer, the vocabulary cut to 2048 so the
    host-side quantisation stays at seconds; KV filled to position 2046, the step run at 2047."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b", num_hidden_layers=1, vocab_size=2048)
    om = mx_oracle(oracle, cfg, seed=1)
    om.fill_kv_synthetic(7, 2047)
    want = om.forward(1234, 2047)
    om.close()
    gap = min_top2_gap(want)
    assert gap >= 2e-3, gap  # otherwise another token id is needed here
    gm = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=1).init()
    gm.fill_kv_synthetic(7, 2047)
    got = gm.forward(1234, 2047)
    gm.close()
    err = float(np.abs(got - want).max())
    print(f"7B layer shapes: max|dlogit| {err:.3e}, oracle top-2 gap {gap:.3e}")
    assert err <= 1e-3, err
    assert int(np.argmax(got)) == int(np.argmax(want))


# ---------------------------------------------------------------- 6. full model properties (no oracle: the lazy
# oracle regenerates its weights per layer and cannot take overwritten ones)
def test_llama7b_full_properties_mxfp4(gpu):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b")
    gm = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=1).init()
    gm.fill_kv_synthetic(7, 2047)
    a = gm.forward(1234, 2047)
    b = gm.forward(1234, 2047)
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)  # deterministic, idempotent step
    st = gm.state()
    assert st["last_argmax"] == int(np.argmax(a)) and st["error"] == 0
    wb, kb = gm.step_bytes()
    D, I, V, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
    elems = L * (4 * D * D + 3 * I * D) + V * D
    assert wb == elems * 0.53125  # cols / 2 + cols / 32 bytes per row
    assert abs(kb - 1.074e9) / 1.074e9 < 0.01
    assert gm.prefill_path() == "decode" and gm.fused_qkv_attn() == 0
    gm.close()


# ---------------------------------------------------------------- 7. tensor parallelism
# Oracle-only scan of this run over seeds 0-7 (minimum top-2 logit gap): 3.8e-3, 3.0e-3, 1.1e-3, 7.5e-4, 2.0e-3,
# 1.8e-3, 3.4e-3, 3.5e-3. Seed 0 has the largest, nearly four times the logit tolerance.
TP_SEED = 0
TP_GAP = 3.77e-3


def test_tp_group_matches_unsharded_oracle(gpu, oracle):
    """Two in-process ranks of tiny-h8 (column shards of wo / down on 32-column blocks) against the unsharded
    oracle. TP_SEED has the largest minimum top-2 gap (TP_GAP) of seeds 0-7 in an oracle-only scan of this run."""
    from simplellminference_amd.model import TPGroup, preset
    otok, olog = _tiny_ref(oracle, "tiny-h8", TP_SEED, "f16")
    assert min_top2_gap(olog) >= 0.9 * TP_GAP
    g = TPGroup(preset("tiny-h8"), tp_size=2, w_dtype="mxfp4", kv_dtype="f16", seed=TP_SEED).init()
    gtok, glog = g.predict(PROMPT, STEPS, want_logits=True)
    g.close()
    err = float(np.abs(glog - olog).max())
    print(f"tiny-h8 TP-2 seed {TP_SEED}: max|dlogit| {err:.3e}")
    assert np.array_equal(gtok, otok), (gtok, otok)
    assert err <= 1e-3, err


# ---------------------------------------------------------------- 8. refusals and fallback
def test_refusals(gpu, monkeypatch):
    from simplellminference_amd._lib import SliError
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    with pytest.raises(SliError, match="fp16"):
        LlamaModel(config=preset("tiny"), w_dtype="mxfp4", seed=0, batch=2).init()
    # a column window off the 32-column blocks: ffn / tp_size = 48 * 11
    with pytest.raises(SliError, match="multiples of 32") as ei:
        TPGroup(preset("tiny-h8", intermediate_size=1056), tp_size=2, w_dtype="mxfp4", seed=0)
    assert ei.value.code == 2  # SLI_ERR_SHAPE
    # the persistent layer stack is fp16 only: a TP shard that fp16 would take is refused at mxfp4
    monkeypatch.setenv("SLI_DEBUG_NOCOMM", "1")
    m = LlamaModel(config=preset("small-h128"), w_dtype="mxfp4", seed=0, tp_rank=0, tp_size=2).init()
    with pytest.raises(SliError, match="fp16 weights"):
        m.set_exec("persist")
    assert m.exec_mode() == "launches"
    m.close()


def test_prefill_falls_back_to_the_decode_step(gpu):
    from simplellminference_amd.model import LlamaModel, preset
    m = LlamaModel(config=preset("tiny-gqa"), w_dtype="mxfp4", kv_dtype="f16", seed=1).init()
    assert m.prefill_path() == "decode"
    a = m.predict(PROMPT + [3, 7], 16)
    m.reset()
    b = m.predict_prefill(PROMPT + [3, 7], 16)
    assert np.array_equal(a, b)
    m.close()
