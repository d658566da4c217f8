"""int8 weights at batch > 1: the MFMA projection from int8 tiles (bgemm.h, sli_matmul_batch_i8) and the batched
model on it, against exact integer products, float64 products and the C oracle (oracle.W_I8).

Bars. The kernel is bit-exact wherever the arithmetic is (small integers; fp16 hi + lo inputs whose every partial
sum is a short multiple of 2^-12), and within 1e-4 (absolute + relative, the fp16 batched projection's bar) of a
float64 product of the dequantised weights otherwise. The model: greedy tokens bit-equal to the oracle's, logits
within 1e-3, the bar of every int8 model test here. The model seeds were chosen with the oracle alone so that its
smallest top-2 logit gap over each run exceeds 2e-3 (a 1e-3 logit difference cannot flip a token); oracle-only scans
of seeds 0-5 (tiny, small-h128-gqa, tiny-h8) and 0-29 (tiny-gqa):
  tiny            seed 4   3.1e-3 (K/V f16), 3.1e-3 (f32)   (seeds 0, 1, 3, 5 stay below 1e-3)
  tiny-gqa        seed 11  2.6e-3 (K/V f16), 2.8e-3 (f32)   (no seed of 0-10 reaches 2e-3)
  small-h128-gqa  seed 3   2.4e-3
  tiny-h8         seed 4   2.2e-3
Each test re-checks its gap on the oracle's logits before it looks at the GPU's.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

PROMPTS = [[1, 17, 42, 99], [5, 6], [300, 2, 77, 8, 9], [11]]  # the ragged prompts of test_gpu_batch.py
PROMPTS8 = PROMPTS + [[7, 3, 250], [64, 65, 66, 67, 68, 69], [2], [123, 45]]
SEED = {"tiny": 4, "tiny-gqa": 11, "small-h128-gqa": 3, "tiny-h8": 4}
MIN_GAP = 2e-3


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ocfg(oracle, cfg):
    return oracle.Config(cfg.vocab_size, cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads,
                         cfg.head_dim, cfg.intermediate_size, cfg.num_hidden_layers, cfg.max_length,
                         cfg.rms_norm_eps, cfg.rope_theta)


def _row_scale(rows):
    return np.exp2((np.arange(rows) % 5) - 2).astype(np.float32)  # 2^((r % 5) - 2): exact in every format here


def _run(torch, x, w, s, tiled):
    from simplellminference_amd import ops
    return ops.matmul_batch_i8(_t(torch, x), _t(torch, w), None if s is None else _t(torch, s), tiled=tiled).cpu().numpy()


# ---------------------------------------------------------------- 1. exact integers
EXACT_SHAPES = [(16, 32, 1),       # one block
                (32, 96, 2),       # K % 64 != 0
                (64, 128, 8),
                (100, 256, 3),     # clamped last tile, idle waves, dead sequence slots
                (48, 4096, 7),     # 8 k-splits, step width 2
                (6144, 4096, 2),   # 3 tiles per workgroup, 2 splits, width 4
                (16032, 4096, 8),  # 4 tiles per workgroup with a short last group
                (4096, 14336, 8)]  # 4 splits, 7 blocks per wave, the 7-wide step


@functools.lru_cache(maxsize=None)
def _exact_case(rows, cols, batch):
    """x integers in [-3, 3], W over the whole int8 range; the int64 product (every partial sum is an integer below
    3 * 128 * 14336 < 2^24: exact in fp32 in any order, and in the float64 BLAS product that computes it here)."""
    r = np.random.default_rng(1000 + rows + cols + batch)
    x = r.integers(-3, 4, (batch, cols)).astype(np.float32)
    w = r.integers(-128, 128, (rows, cols)).astype(np.int8)
    w[0, 0], w[0, 1] = -128, 127
    prod = x.astype(np.float64) @ w.astype(np.float64).T
    want = prod.astype(np.int64)
    assert np.array_equal(want.astype(np.float64), prod) and np.abs(want).max() < 2 ** 24
    return x, w, want


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("rows,cols,batch", EXACT_SHAPES)
def test_exact_integers(gpu, rows, cols, batch, tiled):
    x, w, want = _exact_case(rows, cols, batch)
    s = _row_scale(rows)
    got = _run(gpu, x, w, s, tiled)
    assert np.array_equal(got, want.astype(np.float32) * s[None, :])


@pytest.mark.parametrize("tiled", [False, True])
def test_exact_integers_null_scale(gpu, tiled):
    x, w, want = _exact_case(64, 128, 8)
    assert np.array_equal(_run(gpu, x, w, None, tiled), want.astype(np.float32))


# ---------------------------------------------------------------- 2. the lo half is carried
@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("rows,cols,batch", [(48, 128, 8), (16, 64, 5), (32, 96, 2)])
def test_lo_half_is_carried(gpu, rows, cols, batch, tiled):
    """x = a + c 2^-12 (a in -2..2, c in -1..1): fp16(x) = a for a != 0, so the lo column holds c 2^-12 and hi + lo
    = x exactly. W in [-15, 15]: every partial sum, in any order, is a multiple of 2^-12 below 2^12, exact in fp32,
    so the result equals the float64 product bit for bit. About half the elements have a non-zero lo; dropping it
    changes more than 98 % of the outputs (numpy, seed 0)."""
    r = np.random.default_rng(0)
    a = r.integers(-2, 3, (batch, cols))
    c = r.integers(-1, 2, (batch, cols))
    x = (a + c * 2.0 ** -12).astype(np.float32)
    w = r.integers(-15, 16, (rows, cols)).astype(np.int8)
    s = _row_scale(rows)
    want = (x.astype(np.float64) @ w.astype(np.float64).T) * s[None, :].astype(np.float64)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    hi_only = (x.astype(np.float16).astype(np.float64) @ w.astype(np.float64).T) * s[None, :]
    assert np.mean(hi_only != want) > 0.9  # the case can tell
    got = _run(gpu, x, w, s, tiled)
    assert np.array_equal(got, want.astype(np.float32))


# ---------------------------------------------------------------- 3. realistic values
@functools.lru_cache(maxsize=None)
def _real_case(rows, cols, batch):
    r = np.random.default_rng(rows + cols + batch)
    x = r.standard_normal((batch, cols)).astype(np.float32)
    wf = (r.standard_normal((rows, cols), dtype=np.float32) / np.float32(np.sqrt(cols)))
    s = (np.abs(wf).max(axis=1) / 127.0).astype(np.float32)  # per-row symmetric, scale = amax / 127
    q = np.clip(np.rint(wf / s[:, None]), -127, 127).astype(np.int8)
    want = (x.astype(np.float64) @ q.astype(np.float64).T) * s[None, :].astype(np.float64)  # the dequantised weights
    return x, q, s, want


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("rows,cols,batch", [(768, 4096, 8), (4096, 512, 8), (4000, 4096, 5), (4096, 14336, 8)])
def test_realistic_values(gpu, rows, cols, batch, tiled):
    x, q, s, want = _real_case(rows, cols, batch)
    got = _run(gpu, x, q, s, tiled)
    err = np.abs(got - want)
    print(f"({rows}, {cols}, {batch}) tiled {tiled}: max err {err.max():.3e}, max |want| {np.abs(want).max():.3f}")
    assert np.all(err <= 1e-4 + 1e-4 * np.abs(want)), err.max()


# ---------------------------------------------------------------- 4. argument checks
def test_argument_checks(gpu):
    """Every bad argument gets the status the fp16 entry gives the same mistake."""
    torch = gpu
    from simplellminference_amd import _lib
    L = _lib.load()
    rows, cols, batch = 64, 128, 4
    x = torch.zeros(batch * cols + 8, dtype=torch.float32, device="cuda")
    w8 = torch.zeros(rows * cols + 32, dtype=torch.int8, device="cuda")
    w16 = torch.zeros(rows * cols + 32, dtype=torch.float16, device="cuda")
    y = torch.zeros(batch * rows, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def both(xp, w8p, w16p, yp, c, b, short=0, null_ws=False):
        out = []
        for tiled in (0, 1):
            n8 = L.sli_matmul_batch_i8_workspace_bytes(rows, cols, 4, tiled)
            ws = torch.zeros(n8 // 4 + 1, dtype=torch.float32, device="cuda")
            out.append(L.sli_matmul_batch_i8(xp, w8p, None, yp, rows, c, b, tiled, None if null_ws else p(ws), n8 - short, None))
        n16 = L.sli_matmul_batch_workspace_bytes(rows, cols, 4)
        ws = torch.zeros(n16 // 4 + 1, dtype=torch.float32, device="cuda")
        ref = L.sli_matmul_batch(xp, w16p, _lib.DT_F16, yp, rows, c, b, None if null_ws else p(ws), n16 - short, None)
        return out, ref

    ARG, SHAPE = 1, 2
    cases = {
        "ok": (both(p(x), p(w8), p(w16), p(y), cols, batch), 0),
        "null x": (both(None, p(w8), p(w16), p(y), cols, batch), ARG),
        "null w": (both(p(x), None, None, p(y), cols, batch), ARG),
        "null y": (both(p(x), p(w8), p(w16), None, cols, batch), ARG),
        "null workspace": (both(p(x), p(w8), p(w16), p(y), cols, batch, null_ws=True), ARG),
        "cols % 32": (both(p(x), p(w8), p(w16), p(y), cols - 16, batch), SHAPE),
        "batch 0": (both(p(x), p(w8), p(w16), p(y), cols, 0), SHAPE),
        "batch 9": (both(p(x), p(w8), p(w16), p(y), cols, 9), SHAPE),
        "misaligned x": (both(p(x, 4), p(w8), p(w16), p(y), cols, batch), ARG),
        "misaligned w": (both(p(x), p(w8, 8), p(w16, 8), p(y), cols, batch), ARG),
        "workspace one byte short": (both(p(x), p(w8), p(w16), p(y), cols, batch, short=1), ARG),
    }
    torch.cuda.synchronize()
    for name, ((got, ref), want) in cases.items():
        assert ref == want, (name, ref)
        assert got == [ref, ref], (name, got, ref)
    # the fp16 entry keeps refusing other weight types
    ws = torch.zeros(L.sli_matmul_batch_workspace_bytes(rows, cols, 4) // 4 + 1, dtype=torch.float32, device="cuda")
    assert L.sli_matmul_batch(p(x), p(w8), _lib.DT_I8, p(y), rows, cols, batch, p(ws), ws.numel() * 4, None) == ARG


# ---------------------------------------------------------------- 5. the model against the oracle
_REF = {}


def _gap(logits):
    s = np.sort(logits, axis=-1)
    return float((s[..., -1] - s[..., -2]).min())


def _oracle_runs(oracle, name, kv, prompts, steps, want_kv=False):
    """Per-sequence oracle tokens, logits (and K/V rows), computed once per run and shared; never modified."""
    key = (name, kv, len(prompts), steps)
    if key not in _REF:
        from simplellminference_amd.model import preset
        cfg = preset(name)
        runs = []
        for p in prompts:
            om = oracle.Model(_ocfg(oracle, cfg), seed=SEED[name], wmode=oracle.W_I8, kv_f16=(kv == "f16"))
            tok, log = om.predict(p, steps)
            k, v = om.kv_cache()
            runs.append((tok, log, k[:, :steps].copy(), v[:, :steps].copy()))
            om.close()
        gap = min(_gap(r[1]) for r in runs)
        assert gap > MIN_GAP, (name, kv, gap)  # the oracle's own margin: the bit-equal token bar is attainable
        _REF[key] = runs
    return _REF[key]


def _check_against_oracle(runs, toks, logits, what):
    worst = 0.0
    for b, (otok, olog, _, _) in enumerate(runs):
        assert np.array_equal(toks[b], otok), (what, b, toks[b], otok)
        worst = max(worst, float(np.abs(logits[b] - olog).max()))
    print(f"{what}: max|dlogit| vs the oracle {worst:.3e}")
    assert worst <= 1e-3, (what, worst)


@pytest.mark.parametrize("name", ["tiny", "tiny-gqa"])
@pytest.mark.parametrize("kv", ["f16", "f32"])
def test_model_parity(gpu, oracle, name, kv):
    from simplellminference_amd.model import LlamaModel, preset
    runs = _oracle_runs(oracle, name, kv, PROMPTS, 36)
    gm = LlamaModel(config=preset(name), w_dtype="i8", kv_dtype=kv, seed=SEED[name], batch=len(PROMPTS)).init()
    toks, logits = gm.predict_batch(PROMPTS, 36, want_logits=True)
    assert all(gm.state(b)["error"] == 0 for b in range(len(PROMPTS)))
    gm.close()
    _check_against_oracle(runs, toks, logits, f"{name} kv {kv}")


def test_model_parity_small_h128_batch8(gpu, oracle):
    """head_dim 128, GQA, batch 8: a width-4 NORM gate/up, a 4-split down and a vocabulary of 1000 whose last logits
    tile is clamped; per-sequence K/V rows within 2e-3 (test_gpu_batch.py test_batch_state_and_history)."""
    from simplellminference_amd.model import LlamaModel, preset
    name, steps = "small-h128-gqa", 24
    cfg = preset(name)
    runs = _oracle_runs(oracle, name, "f16", PROMPTS8, steps)
    gm = LlamaModel(config=cfg, w_dtype="i8", kv_dtype="f16", seed=SEED[name], batch=8).init()
    toks, logits = gm.predict_batch(PROMPTS8, steps, want_logits=True)
    _check_against_oracle(runs, toks, logits, name)
    for b, (_, _, ok, ov) in enumerate(runs):
        assert gm.state(b)["error"] == 0 and gm.state(b)["pos"] == steps
        for layer in range(cfg.num_hidden_layers):
            np.testing.assert_allclose(gm.kv(layer, 0, steps, seq=b), ok[layer], rtol=0, atol=2e-3)
            np.testing.assert_allclose(gm.kv(layer, 1, steps, seq=b), ov[layer], rtol=0, atol=2e-3)
    gm.close()


# ---------------------------------------------------------------- 6. the two layouts agree
def test_layouts_agree(gpu, oracle, monkeypatch):
    """The fragment-layout copies and the row-major fallback (SLI_DEBUG_BG_ROWMAJOR) both meet the oracle's bar. The
    two paths run the same kernel on the same plan: the same blocks per wave, the same wave and split order, so the
    same fp32 sums, and the logits are compared bit for bit."""
    from simplellminference_amd.model import LlamaModel, preset
    name = "tiny-gqa"
    runs = _oracle_runs(oracle, name, "f16", PROMPTS, 36)
    out = []
    for rowmajor in (False, True):
        if rowmajor:
            monkeypatch.setenv("SLI_DEBUG_BG_ROWMAJOR", "1")
        gm = LlamaModel(config=preset(name), w_dtype="i8", kv_dtype="f16", seed=SEED[name], batch=len(PROMPTS)).init()
        toks, logits = gm.predict_batch(PROMPTS, 36, want_logits=True)
        gm.close()
        _check_against_oracle(runs, toks, logits, f"{name} row-major {rowmajor}")
        out.append((toks, logits))
    print(f"tiled vs row-major: max|dlogit| {float(np.abs(out[0][1] - out[1][1]).max()):.3e}")
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])


# ---------------------------------------------------------------- 7. weights replaced
def test_weights_replaced(gpu, oracle):
    """set_weight on one matrix of a batch-2 int8 model after a first step: the tiles are rebuilt (the logits change
    and equal, bit for bit, those of a fresh model given the same weights before its first step), and the matrix
    reads back as its int8 dequantisation."""
    from simplellminference_amd.model import LlamaModel, preset
    from simplellminference_amd.tp import KINDS
    cfg = preset("tiny-gqa")
    prompts = PROMPTS[:2]
    om = oracle.Model(_ocfg(oracle, cfg), seed=5, wmode=oracle.W_F32)
    w_new = om.weight(oracle.T_WO, 0).copy()
    om.close()
    gm = LlamaModel(config=cfg, w_dtype="i8", kv_dtype="f16", seed=SEED["tiny-gqa"], batch=2).init()
    _, before = gm.predict_batch(prompts, 12, want_logits=True)
    gm.set_weight(KINDS["wo"], 0, w_new)
    gm.reset()
    _, after = gm.predict_batch(prompts, 12, want_logits=True)
    deq = np.empty_like(w_new)
    for i in range(w_new.shape[0]):
        q, s = oracle.quant_row_i8(w_new[i])
        deq[i] = q.astype(np.float32) * np.float32(s)
    assert np.array_equal(gm.weight_shard(KINDS["wo"], 0), deq)
    gm.close()
    fm = LlamaModel(config=cfg, w_dtype="i8", kv_dtype="f16", seed=SEED["tiny-gqa"], batch=2).init()
    fm.set_weight(KINDS["wo"], 0, w_new)
    _, fresh = fm.predict_batch(prompts, 12, want_logits=True)
    fm.close()
    assert not np.array_equal(before, after)
    assert np.array_equal(after, fresh)


# ---------------------------------------------------------------- 8. tensor parallelism
def test_tp_group_matches_unsharded_oracle(gpu, oracle):
    from simplellminference_amd.model import TPGroup, preset
    name = "tiny-h8"
    runs = _oracle_runs(oracle, name, "f16", PROMPTS, 36)
    g = TPGroup(preset(name), 2, w_dtype="i8", kv_dtype="f16", seed=SEED[name], batch=4).init()
    toks, logits = g.predict_batch(PROMPTS, 36, want_logits=True)
    g.close()
    _check_against_oracle(runs, toks, logits, f"{name} TP-2 group")


@pytest.mark.parametrize("mode", ["fused_wg", "oneshot"])
def test_two_rank_processes(gpu, mode):
    """Two rank processes on one device, int8 at batch 2, exchanging through the one-shot buffers only (the pattern
    and helper of test_gpu_tp.py test_oneshot_allreduce_two_processes; seed 0, whose oracle top-2 gap over these
    prompts is 4.6e-3): tokens equal to the TP-1 int8 model's, logits within 1e-3, no device error. fused_wg runs
    the exchange inside the MFMA wo / down (BgEpiPush, with the row scales)."""
    from tests.test_gpu_tp import _oneshot_rank, _port, _preset, _prompts
    from simplellminference_amd.model import LlamaModel
    name, batch = "tiny-gqa", 2
    ref = LlamaModel(config=_preset(name), w_dtype="i8", kv_dtype="f16", seed=0, batch=batch).init()
    rtoks, rlogits = ref.predict_batch(_prompts(batch), 16, want_logits=True)
    ref.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_oneshot_rank, args=(r, 2, port, name, batch, q, mode, "i8")) for r in range(2)]
    for p in procs:
        p.start()
    status, toks, logits, err = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
    assert status == "ok", toks
    assert err == 0
    assert np.array_equal(toks, rtoks)
    assert np.abs(logits - rlogits).max() <= 1e-3


# ---------------------------------------------------------------- 9. refusals kept
def test_refusals_kept(gpu):
    from simplellminference_amd._lib import SliError
    from simplellminference_amd.model import LlamaModel, preset
    for w in ("f32", "mxfp4"):
        with pytest.raises(SliError, match="fp16"):
            LlamaModel(config=preset("tiny"), w_dtype=w, seed=0, batch=2).init()
    m = LlamaModel(config=preset("tiny-gqa"), w_dtype="i8", kv_dtype="f16", seed=0, batch=2).init()
    with pytest.raises(SliError):
        m.set_exec("persist")
    assert m.exec_mode() == "launches"
    assert m.prefill_path() == "decode"
    m.close()
