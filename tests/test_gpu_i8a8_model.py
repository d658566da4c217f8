"""The model path of the integer-MFMA prefill: LlamaModel.set_prefill("gemm-i8a8") (SLI_PREFILL_GEMM_I8A8), on the tiny
presets, whose projection depths (256, 768) lie on 128."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _prompt(n, vocab, seed=3):
    return [int(t) for t in np.random.default_rng(seed + n).integers(0, vocab, n)]


def _model(w="i8", kv="f16", name="tiny-gqa", seed=7, **over):
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
    made = [_model(w="f16"), _model(w="mxfp4"), _model(kv="f32"),
            LlamaModel(config=preset("tiny-gqa"), w_dtype="i8", kv_dtype="f16", seed=7, batch=2).init(),
            TPGroup(preset("tiny-h8"), tp_size=2, w_dtype="i8", kv_dtype="f16", seed=5).init()]
    for m in made:
        with pytest.raises(SliError) as e:
            m.set_prefill("gemm-i8a8")
        assert e.value.code == 7 and "set_prefill" in str(e.value), e.value  # SLI_ERR_STATE, with the reason
        m.close()
    m = _model(kv="f8")  # accepted, and a prompt runs through the FP8-cache epilogue and attention behind it
    rows, logits = _run(m, _prompt(40, m.config.vocab_size), "gemm-i8a8")
    m.close()
    assert np.isfinite(rows).all() and np.isfinite(logits).all() and np.abs(rows).max() > 0


def test_split_equals_whole(gpu):
    """30 tokens at once against 20 and extend_one from position 19 (32-row chunks all): bit for bit."""
    m = _model()
    prompt = _prompt(30, m.config.vocab_size)
    whole = _run(m, prompt, "gemm-i8a8")
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
    """The mode is its own arithmetic (rows and logits differ from "gemm"), ||i8a8 - gemm|| < ||gemm - f16|| on the
    first-step logits (the activation rounding costs less than the int8 weights already do), and gemm -> gemm-i8a8 ->
    gemm repeats the first gemm result bit for bit."""
    m = _model()
    prompt = _prompt(40, m.config.vocab_size)
    g1, a8, g2 = (_run(m, prompt, mode) for mode in ("gemm", "gemm-i8a8", "gemm"))
    m.close()
    h = _model(w="f16")
    f16 = _run(h, prompt, "gemm")
    h.close()
    assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1])
    assert not np.array_equal(a8[0], g1[0]) and not np.array_equal(a8[1], g1[1])
    d_a8, d_w = float(np.linalg.norm(a8[1] - g1[1])), float(np.linalg.norm(g1[1] - f16[1]))
    print(f"||i8a8 - gemm|| {d_a8:.6g}  ||gemm - f16|| {d_w:.6g}")
    assert d_a8 < d_w, (d_a8, d_w)
