"""Seeded temperature / top-k / top-p sampling on the GPU (csrc/sample.h; the rule: sli.h at sli_sample): the op
over small and production vocabularies, the edge rows, determinism and the draw's counter, then the engine: sampling
inside the captured step for batch 1 and batch 4 over three weight / cache formats, after a GEMM prefill, switched off
again, and the refusals.

Every token is judged by tests/sample_ref.py's acceptance test (derived there, not tuned): inside the float64 nucleus at
top_p + 1e-4, and its float64 key within 8 * 2^-23 * max(1, max |key|) of the best key over the nucleus at top_p - 1e-4.
With top-k alone the token is additionally inside the exact C_k.
"""
import numpy as np
import pytest

from tests import sample_ref as R

pytestmark = pytest.mark.gpu


def _logits(seed, rows, V, ties=True):
    rng = np.random.default_rng(seed)
    l = rng.normal(0, 2.5, (rows, V)).astype(np.float32)
    if ties and V >= 8:
        l[:, V // 3:V // 3 + 4] = l[:, V // 3:V // 3 + 1]  # a run of four equal values
    return l


def _sample(torch, ops, l, T, k, p, seed, pos, seq0=0, stride="V", rows=None):
    """ops.sample over the rows of l (numpy [rows, V], or [V] drawn `rows` times with row_stride 0). stride "V":
    contiguous rows; "pad": rows V + 3 floats apart (so most rows start off 16-byte alignment)."""
    dev = torch.device("cuda")
    if l.ndim == 1:
        t = torch.from_numpy(l).to(dev).unsqueeze(0).expand(rows, l.size)
    elif stride == "pad":
        buf = torch.full((l.shape[0], l.shape[1] + 3), float("nan"), device=dev)
        buf[:, :l.shape[1]] = torch.from_numpy(l).to(dev)
        t = buf[:, :l.shape[1]]
    else:
        t = torch.from_numpy(l).to(dev)
    n = t.shape[0]
    pos_t = torch.from_numpy(np.broadcast_to(np.asarray(pos, np.int32), (n,)).copy()).to(dev)
    out = ops.sample(t, T, k, p, seed, pos_t, seq0=seq0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(toks, l, T, k, p, seed, pos, seq0=0, what=""):
    """Every toks[r] accepted as the draw of row r (l [rows, V], or [V] shared by all rows)."""
    shared = R.Acceptor(l, T, k, p) if l.ndim == 1 else None
    pos = np.broadcast_to(np.asarray(pos), (len(toks),))
    for r, t in enumerate(toks):
        a = shared or R.Acceptor(l[r], T, k, p)
        ok, why = a.check(t, seed, seq0 + r, int(pos[r]))
        assert ok, (what, "row", r, (T, k, p), why)
        if p >= 1.0 and not a.degenerate:
            assert a.ck[int(t)], (what, "row", r, "outside the exact top-k set")


# ---------------------------------------------------------------- the op, small vocabularies
def _small_settings(V):
    s = [(1.0, 0, 1.0), (0.5, 0, 1.0)]
    s += [(1.0, k, 1.0) for k in (1, 2, V - 1, V, V + 5) if k >= 1]
    s += [(1.0, 0, p) for p in (1e-6, 0.3, 0.9)]
    s += [(0.7, max(1, V // 4), 0.9), (1.3, 7, 0.3), (1.0, 2, 1e-6)]
    return s


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1000, 1025])
def test_op_small_vocabularies(gpu, V):
    from simplellminference_amd import ops
    rows = 256
    l = _logits(V, rows, V)
    pos = (np.arange(rows) * 7 + 3).astype(np.int32)
    for T, k, p in _small_settings(V):
        for stride in ("V", "pad"):
            toks = _sample(gpu, ops, l, T, k, p, 17, pos, seq0=2, stride=stride)
            _check(toks, l, T, k, p, 17, pos, seq0=2, what=f"V={V} stride={stride}")
        toks = _sample(gpu, ops, l[5], T, k, p, 17, pos, seq0=2, rows=rows)
        _check(toks, l[5], T, k, p, 17, pos, seq0=2, what=f"V={V} stride=0")


# ---------------------------------------------------------------- the op, the workloads' vocabularies
BIG = {}


def _big(V):
    if V not in BIG:
        BIG[V] = _logits(1000 + V, 1, V)[0]
    return BIG[V]


@pytest.mark.parametrize("V,rows", [(32000, 200), (128256, 64)])
@pytest.mark.parametrize("T,k,p", [(1.0, 0, 0.9), (0.7, 50, 0.5), (1.3, 40, 1.0), (0.3, 0, 0.3), (1.0, 1000, 0.95)])
def test_op_workload_vocabularies(gpu, V, rows, T, k, p):
    from simplellminference_amd import ops
    l = _big(V)
    toks = _sample(gpu, ops, l, T, k, p, 5, 11, rows=rows)
    _check(toks, l, T, k, p, 5, 11, what=f"V={V}")


def test_op_is_bitwise_deterministic(gpu):
    from simplellminference_amd import ops
    l = _big(128256)
    runs = [_sample(gpu, ops, l, 1.0, 0, 0.9, 5, 11, rows=64) for _ in range(3)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


def test_op_counter_sequence_and_seed(gpu):
    """pos, seq0 and seed each change the uniforms exactly as the reference says: the tokens are the reference's under
    each, and they move."""
    from simplellminference_amd import ops
    l = _big(32000)
    T, k, p, rows = 1.0, 200, 0.95, 64
    base = _sample(gpu, ops, l, T, k, p, 5, 11, rows=rows)
    _check(base, l, T, k, p, 5, 11)
    for seed, pos, seq0 in ((5, 12, 0), (5, 11, 1), (6, 11, 0), (5, 2 ** 31 - 1, 0), (5, 11, 65536 - 8), (2 ** 32 - 1, 0, 0)):
        toks = _sample(gpu, ops, l, T, k, p, seed, pos, seq0=seq0, rows=rows)
        _check(toks, l, T, k, p, seed, pos, seq0=seq0, what=f"seed={seed} pos={pos} seq0={seq0}")
        assert not np.array_equal(toks, base)
    # sequence ids wrap at 16 bits; row r of seq0 = 1 is row r + 1 of seq0 = 0
    shifted = _sample(gpu, ops, l, T, k, p, 5, 11, seq0=1, rows=rows)
    assert np.array_equal(shifted[:-1], base[1:])
    # positions are read per row from the device, through pos_stride
    torch = gpu
    pos2 = torch.arange(2 * rows, dtype=torch.int32, device="cuda")[::2]
    t = torch.from_numpy(l).cuda().unsqueeze(0).expand(rows, l.size)
    toks = ops.sample(t, T, k, p, 5, pos2).cpu().numpy()
    _check(toks, l, T, k, p, 5, np.arange(rows) * 2)


# ---------------------------------------------------------------- edges
def _one(gpu, l, T=1.0, k=0, p=1.0, seed=3, pos=4, rows=32):
    from simplellminference_amd import ops
    l = np.asarray(l, np.float32)
    toks = _sample(gpu, ops, l, T, k, p, seed, pos, rows=rows)
    _check(toks, l, T, k, p, seed, pos)
    return toks


def _argmax(gpu, l):
    from simplellminference_amd import ops
    return int(ops.argmax(gpu.from_numpy(np.asarray(l, np.float32)).cuda()).cpu())


def test_edge_all_equal_logits(gpu):
    for V in (5, 777):
        for k, p in ((0, 1.0), (3, 1.0), (0, 0.5), (3, 0.01)):
            toks = _one(gpu, np.full(V, 1.25, np.float32), k=k, p=p)
            assert len(set(toks.tolist())) > 1  # every index stays a candidate


def test_edge_ties_across_the_k_boundary(gpu):
    l = np.full(300, -4.0, np.float32)
    l[[7, 70, 170, 270]] = 0.0
    l[[70, 270]] = -0.0  # +-0 are one value
    l[9] = 2.0
    for k in (2, 3, 4, 5):
        toks = _one(gpu, l, k=k, rows=128)
        assert set(toks.tolist()) == {7, 9, 70, 170, 270}
    assert set(_one(gpu, l, k=1, rows=16).tolist()) == {9}
    # p cuts inside the tie: the whole tie enters
    toks = _one(gpu, l, T=1.0, p=0.6, rows=128)  # e^2 alone is 0.44 of the mass, with the four zeros 0.68
    assert set(toks.tolist()) == {7, 9, 70, 170, 270}


def test_edge_nan_and_minus_inf_are_never_chosen(gpu):
    rng = np.random.default_rng(9)
    l = rng.normal(0, 1, 1000).astype(np.float32)
    bad = rng.choice(1000, 600, replace=False)
    l[bad[:300]] = np.nan
    l[bad[300:]] = -np.inf
    l[0] = np.nan
    for k, p in ((0, 1.0), (500, 1.0), (999, 1.0), (0, 0.999), (450, 0.9)):
        toks = _one(gpu, l, T=2.0, k=k, p=p, rows=256)
        assert np.isfinite(l[toks]).all()
        assert len(set(toks.tolist())) > 20


def test_edge_single_finite_logit_and_last_index(gpu):
    for V in (1, 6, 1024, 1029, 4099):
        l = np.full(V, -np.inf, np.float32)
        l[V - 1] = -3.0  # the last index as the only candidate
        for k, p in ((0, 1.0), (1, 1.0), (0, 0.5), (2, 0.5)):
            assert set(_one(gpu, l, k=k, p=p, rows=8).tolist()) == {V - 1}
        l[:] = np.nan
        l[V // 2] = 1e30
        assert set(_one(gpu, l, T=0.01, p=0.9, rows=8).tolist()) == {V // 2}


def test_edge_degenerate_rows_equal_argmax(gpu):
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(4)
    rows = [np.full(100, nan), np.full(100, -inf), np.r_[np.full(50, -inf), np.full(50, nan)],
            np.r_[np.full(50, nan), np.full(50, -inf)]]
    a = rng.normal(0, 1, 5000)
    a[[1234, 4321]] = inf
    rows.append(a)
    b = a.copy()
    b[0] = nan  # a NaN at index 0 is never displaced (sli_argmax's scan)
    rows.append(b)
    for l in rows:
        l = l.astype(np.float32)
        for k, p in ((0, 1.0), (10, 0.5)):
            toks = _one(gpu, l, k=k, p=p, rows=4)
            assert set(toks.tolist()) == {_argmax(gpu, l)} == {R.argmax_a8(l)}


def test_edge_large_scaled_logits(gpu):
    """|l / T| up to 1e4: the masses underflow to zero far from the maximum and the keys are large."""
    rng = np.random.default_rng(6)
    l = rng.uniform(-100, 100, 3000).astype(np.float32)
    l[[5, 2999]] = 100.0
    for T, k, p in ((0.01, 0, 1.0), (0.01, 0, 0.9), (0.01, 100, 0.5), (0.02, 3, 1.0)):
        _one(gpu, l, T=T, k=k, p=p, rows=64)
    big = (rng.uniform(-1, 1, 3000) * 1e6).astype(np.float32)
    _one(gpu, big, T=100.0, k=0, p=0.8, rows=64)


def test_edge_top_k_one_is_argmax(gpu):
    l = np.random.default_rng(8).permutation(5000).astype(np.float32)  # untied
    for T, p in ((1.0, 1.0), (100.0, 1.0), (0.5, 0.3)):
        assert set(_one(gpu, l, T=T, k=1, p=p, rows=16).tolist()) == {_argmax(gpu, l)}


# ---------------------------------------------------------------- the engine
STEPS = 36
PROMPTS = [[5, 17, 300, 42, 9], [511], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [77, 78]]
MODELS = [("tiny", 1, "f16", "f16", (0.05, 40, 0.9)), ("tiny-gqa", 4, "f16", "f16", (0.05, 0, 0.8)),
          ("tiny", 1, "i8", "f8", (0.02, 0, 0.7)), ("tiny-gqa", 4, "i8", "f8", (0.03, 25, 1.0)),
          ("tiny", 1, "mxfp4", "f16", (0.1, 20, 0.95))]


def _model(name, B, w, kv, seed=3):
    from simplellminference_amd.model import LlamaModel, preset
    return LlamaModel(config=preset(name), w_dtype=w, kv_dtype=kv, seed=seed, batch=B).init()


def _run(m, B, prompts, prefill=False):
    """tokens [B, STEPS], logits [B, STEPS, V]"""
    if B == 1:
        f = m.predict_prefill if prefill else m.predict
        toks, logits = f(prompts[0], STEPS, want_logits=True)
        return toks[None], logits[None]
    return m.predict_batch(prompts, STEPS, want_logits=True)


def _check_run(toks, logits, prompts, prm, seed, first=0):
    """Positions past the prompt hold accepted draws from the step before (as sequence b at that position); prompt
    tokens are fed unchanged. first: the first position whose logits exist (a prefill computes none before it)."""
    T, k, p = prm
    for b, prompt in enumerate(prompts):
        assert toks[b, :len(prompt)].tolist() == prompt[:STEPS]
        for t in range(max(len(prompt) - 1, first), STEPS - 1):
            ok, why = R.accept(toks[b, t + 1], logits[b, t], T, k, p, seed, b, t)
            assert ok, ("sequence", b, "position", t, why)


@pytest.mark.parametrize("name,B,w,kv,prm", MODELS)
def test_model_samples_inside_the_step(gpu, name, B, w, kv, prm):
    T, k, p = prm
    prompts = PROMPTS[:B]
    m = _model(name, B, w, kv)
    greedy_toks, greedy_logits = _run(m, B, prompts)
    assert m.sampling() is None and m.sampled() == -1
    m.set_sampling(T, top_k=k, top_p=p, seed=21)
    got = m.sampling()
    assert (got["top_k"], got["seed"]) == (k, 21) and got["temperature"] == np.float32(T)
    toks, logits = _run(m, B, prompts)
    _check_run(toks, logits, prompts, prm, 21)
    assert not np.array_equal(toks, greedy_toks)
    for b in range(B):
        # the state after the last step: the draw from the last logits was fed and recorded; last_argmax stays greedy
        hist = m.history(b, STEPS + 1)
        assert np.array_equal(hist[:STEPS], toks[b]) and m.sampled(b) == hist[STEPS] == m.state(b)["token"]
        ok, why = R.accept(hist[STEPS], logits[b, STEPS - 1], T, k, p, 21, b, STEPS - 1)
        assert ok, why
        assert m.state(b)["last_argmax"] == R.argmax_a8(logits[b, STEPS - 1])
    # the same seed: the same run, bit for bit; another seed: the reference's other run
    toks2, logits2 = _run(m, B, prompts)
    assert np.array_equal(toks2, toks) and np.array_equal(logits2.view(np.uint32), logits.view(np.uint32))
    captures = m.graph_captures()
    m.set_sampling(T, top_k=k, top_p=p, seed=22)
    toks3, logits3 = _run(m, B, prompts)
    _check_run(toks3, logits3, prompts, prm, 22)
    assert not np.array_equal(toks3, toks)
    assert m.graph_captures() == captures  # new parameters: no new graph
    # an idempotent step draws the same token twice
    for b in range(B):
        m.set_state_seq(b, int(toks[b, 20]), 20, advance=False)
    m.step()
    first = [m.sampled(b) for b in range(B)]
    m.step()
    assert [m.sampled(b) for b in range(B)] == first
    step_logits = m.logits()[0].reshape(B, -1)
    for b in range(B):
        ok, why = R.accept(first[b], step_logits[b], T, k, p, 22, b, 20)
        assert ok, why
        assert m.state(b)["pos"] == 20 and m.state(b)["token"] == toks[b, 20]
    # back to greedy: the model's greedy run in tokens and logits bits, and the sampled run, fed as a prompt,
    # reproduces the sampling run's logits bit for bit
    m.set_sampling(None)
    assert m.sampling() is None and m.sampled() == -1
    again_toks, again_logits = _run(m, B, prompts)
    assert m.graph_captures() == captures + 1  # sampling off: the greedy graph is recorded again
    assert np.array_equal(again_toks, greedy_toks)
    assert np.array_equal(again_logits.view(np.uint32), greedy_logits.view(np.uint32))
    forced_toks, forced_logits = _run(m, B, [toks[b].tolist() for b in range(B)])
    assert np.array_equal(forced_toks, toks)
    assert np.array_equal(forced_logits.view(np.uint32), logits.view(np.uint32))
    m.close()


@pytest.mark.parametrize("w,kv,mode", [("f16", "f16", "gemm"), ("i8", "f8", "gemm-kv8"), ("mxfp4", "f16", "decode")])
def test_model_samples_after_prefill(gpu, w, kv, mode):
    prm = (0.05, 30, 0.9)
    prompt = [(7 * i + 3) % 512 for i in range(12)]
    m = _model("tiny", 1, w, kv)
    m.set_prefill(mode)
    m.set_sampling(prm[0], top_k=prm[1], top_p=prm[2], seed=9)
    toks, logits = _run(m, 1, [prompt], prefill=True)
    assert np.isnan(logits[0, :len(prompt) - 1]).all()
    _check_run(toks, logits, [prompt], prm, 9, first=len(prompt) - 1)
    assert m.sampled() == m.history(0, STEPS + 1)[STEPS]
    m.close()


def test_model_sampling_parameters_are_checked(gpu):
    from simplellminference_amd import SliError
    m = _model("tiny", 1, "f16", "f16")
    for kw in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=1e3),
               dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_p=1.5), dict(temperature=1.0, top_k=-2)):
        with pytest.raises(SliError) as e:
            m.set_sampling(**kw)
        assert e.value.code == 1
    assert m.sampling() is None
    m.set_sampling(0.0)  # temperature 0: greedy
    assert m.sampling() is None and m.graph_captures() == 0
    m.close()


def test_model_sampling_refusals(gpu, monkeypatch):
    from simplellminference_amd import SliError
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    g = TPGroup(preset("tiny"), 2, seed=1).init()
    with pytest.raises(SliError, match="in-process tp group") as e:
        g.ranks[1].set_sampling(1.0)
    assert e.value.code == 7
    g.close()
    monkeypatch.setenv("SLI_DEBUG_NOCOMM", "1")
    m = LlamaModel(config=preset("tiny"), w_dtype="f16", kv_dtype="f16", seed=1, tp_rank=1, tp_size=2).init()
    with pytest.raises(SliError, match="tp_size > 1") as e:
        m.set_sampling(1.0)
    assert e.value.code == 7
    m.close()
    monkeypatch.delenv("SLI_DEBUG_NOCOMM")
    # the persistent layers, in either order of the two setters
    m = LlamaModel(config=preset("small-h128"), w_dtype="f16", kv_dtype="f16", seed=1).init()
    m.set_exec("persist")
    with pytest.raises(SliError, match="persistent layers") as e:
        m.set_sampling(1.0)
    assert e.value.code == 7 and m.sampling() is None
    m.set_exec("launches")
    m.set_sampling(1.0, top_k=5)
    with pytest.raises(SliError, match="sampling is on") as e:
        m.set_exec("persist")
    assert e.value.code == 7 and m.exec_mode() == "launches"
    toks = m.predict([1, 2, 3], 8)
    assert toks[:3].tolist() == [1, 2, 3]
    m.close()
