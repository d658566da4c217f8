"""Scoring prompts through the GEMM prefill (sli_model_score_seqs; LlamaModel.score / perplexity): per-token
log-probabilities from the chunk rows' final norm, the role-3 LM-head GEMM and the group-table score launch.

Reference: the oracle's predict(p, len(p)) logits at positions 0 .. n - 2 put through tests/score_ref.py (position t
scores token p[t + 1]). Bars, both from the project's 1e-3 logit bar (lse and max are 1-Lipschitz in the max norm):
|d logprob| <= 2e-3 and |d top_logprob| <= 2e-3, the latter also where `top` differs (it compares two maxima). `top`
follows tests/test_gpu_batch_prefill.py: equal wherever the oracle's top-2 gap exceeds 2e-3, and at most 5 % of the
scored positions may be left out; each case also states how many the oracle alone leaves out (seeds chosen with the
oracle alone, on the CPU), and no more than that are.
"""
import numpy as np
import pytest

from tests import score_ref as R
from tests.test_gpu_batch_prefill import _ocfg, _prompt

pytestmark = pytest.mark.gpu

BAR, GAP = 2e-3, 2e-3
LENS = (1, 2, 17, 40)


def _ref_from_logits(p, logits):
    """logits [>= n - 1, V] of positions 0 ..: (logprob, top, top_logprob, top-2 gap) for tokens 1 .. n - 1."""
    n = len(p)
    lp, top, tlp = R.score_rows(logits[:n - 1], p[1:]) if n > 1 else (np.zeros(0), np.zeros(0, np.int32), np.zeros(0))
    gap = np.array([R.top2_gap(logits[t]) for t in range(n - 1)])
    return lp, top, tlp, gap


_ORACLE = {}


def _oracle_refs(oracle, name, cfg, prompts, seed, wmode=None):
    key = (name, tuple(map(tuple, prompts)), seed, wmode)
    if key not in _ORACLE:
        out = []
        for p in prompts:
            if len(p) < 2:
                out.append(_ref_from_logits(p, np.zeros((0, cfg.vocab_size), np.float32)))
                continue
            om = oracle.Model(_ocfg(oracle, cfg), seed=seed, wmode=oracle.W_F16 if wmode is None else wmode, kv_f16=True)
            _, log = om.predict(p, len(p))
            om.close()
            out.append(_ref_from_logits(p, log))
        _ORACLE[key] = out
    return _ORACLE[key]


def _hold(recs, prompts, refs, may_leave_out, tag):
    left = total = 0
    e1 = e2 = 0.0
    for b, (rec, p, (lp, top, tlp, gap)) in enumerate(zip(recs, prompts, refs)):
        n = len(p)
        assert rec["logprobs"].shape == rec["top"].shape == rec["top_logprobs"].shape == (n - 1,), b
        if n < 2:
            continue
        e1 = max(e1, float(np.abs(rec["logprobs"] - lp).max()))
        e2 = max(e2, float(np.abs(rec["top_logprobs"] - tlp).max()))
        clear = gap > GAP
        assert np.array_equal(rec["top"][clear], top[clear]), (tag, b)
        left += int((~clear).sum())
        total += n - 1
    print(f"{tag}: max|d logprob| {e1:.3e}, max|d top_logprob| {e2:.3e}, {left} of {total} positions left out of top")
    assert e1 <= BAR and e2 <= BAR, (tag, e1, e2)
    assert left <= may_leave_out and left <= 0.05 * total, (tag, left, total)


# (config, overrides, weights, oracle weight mode, seed, prompt lengths, positions the oracle alone leaves out)
CASES = {
    "a": ("tiny", {}, "f16", None, 6, LENS, 0),
    "b": ("tiny-gqa", {}, "f16", None, 2, LENS, 0),
    "c": ("tiny-gqa", {}, "i8", "W_I8", 1, LENS, 0),
    "d": ("tiny-gqa", dict(max_length=320), "f16", None, 3, (300, 5, 129, 33), 5),  # two chunks, one sequence in both
    "e": ("small-h128-gqa", {}, "f16", None, 2, (3, 60, 17, 33), 1),                # vocab 1000, head_dim 128
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_score_matches_oracle(gpu, oracle, case):
    from simplellminference_amd.model import LlamaModel, preset
    name, over, w, wmode, seed, lens, may = CASES[case]
    cfg = preset(name, **over)
    prompts = [_prompt(n, cfg.vocab_size) for n in lens]
    gm = LlamaModel(config=cfg, w_dtype=w, kv_dtype="f16", seed=seed, batch=4).init()
    assert gm.score_ok()
    recs = gm.score(prompts)
    gm.close()
    refs = _oracle_refs(oracle, name + str(over), cfg, prompts, seed, getattr(oracle, wmode) if wmode else None)
    _hold(recs, prompts, refs, may, f"case {case}")


@pytest.mark.parametrize("kw,seed", [(dict(w_dtype="mxfp4", kv_dtype="f16", mx_batch=True), 7),
                                     (dict(w_dtype="f16", kv_dtype="f8"), 0)], ids=["mxfp4", "fp8-cache"])
def test_score_matches_own_decode_route(gpu, kw, seed):
    """Case f: MXFP4 weights and an FP8 cache against the same model's own teacher-forced predict_batch logits; the
    same bars and the same 5 % condition on the decode route's own near ties. Measured on an MI355X with the seeds
    as given (7 and 0, no scan needed): the decode route's logits leave 0 of 56 positions out for MXFP4 and 1 of 56 for
    the FP8 cache; max |d logprob| 2.7e-5 and 8.5e-7."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    prompts = [_prompt(n, cfg.vocab_size) for n in LENS]
    gm = LlamaModel(config=cfg, seed=seed, batch=4, **kw).init()
    _, logits = gm.predict_batch(prompts, max(LENS), want_logits=True)
    gm.reset()
    recs = gm.score(prompts)
    gm.close()
    refs = [_ref_from_logits(p, logits[b]) for b, p in enumerate(prompts)]
    total = sum(len(p) - 1 for p in prompts)
    _hold(recs, prompts, refs, int(0.05 * total), "case f " + kw["w_dtype"] + "/" + kw["kv_dtype"])


def _raw_score(gm, prompts):
    """sli_model_score_seqs itself: the whole [n_seqs][ld] host arrays, sentinels and all."""
    import ctypes
    from simplellminference_amd._lib import call
    P, lens, ld = gm._ragged(prompts)
    seqs = np.arange(len(prompts), dtype=np.int32)
    lp = np.zeros((len(prompts), ld), np.float32)
    top = np.zeros((len(prompts), ld), np.int32)
    tlp = np.zeros((len(prompts), ld), np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call("sli_model_score_seqs", gm._h, vp(seqs), seqs.size, vp(P), vp(lens), ld, vp(lp), vp(top), vp(tlp))
    return lp, top, tlp


def _snap(gm, L, upto):
    return ([[gm.kv(layer, which, upto, seq=b) for layer in range(L) for which in (0, 1)] for b in range(gm.batch)],
            [gm.state(b) for b in range(gm.batch)])


def test_score_leaves_what_prefill_batch_leaves(gpu, oracle):
    """Case g: K/V rows, state, history and the greedy continuation after score() are those after prefill_batch();
    entry 0 is NaN / -1 / NaN, a length-1 prompt scores nothing, and a second call with other lengths (another chunk
    size, fewer sequences) gives the oracle's values again."""
    from simplellminference_amd.model import LlamaModel, preset
    name, _, w, _, seed, lens, may = CASES["b"]
    cfg = preset(name)
    L = cfg.num_hidden_layers
    prompts = [_prompt(n, cfg.vocab_size) for n in lens]
    gm = LlamaModel(config=cfg, w_dtype=w, kv_dtype="f16", seed=seed, batch=4).init()
    out = []
    for route in ("score", "prefill_batch"):
        gm.reset()
        recs = getattr(gm, route)(prompts)
        if route == "score":
            lp, top, tlp = _raw_score(gm, prompts)  # (scoring again leaves the same rows and state)
            assert np.isnan(lp[:, 0]).all() and (top[:, 0] == -1).all() and np.isnan(tlp[:, 0]).all()
            for b, n in enumerate(lens):  # and everything past the prompt
                assert np.isnan(lp[b, n:]).all() and (top[b, n:] == -1).all() and np.isnan(tlp[b, n:]).all()
                assert not np.isnan(lp[b, 1:n]).any() and (top[b, 1:n] >= 0).all()
                assert np.array_equal(lp[b, 1:n], recs[b]["logprobs"]) and np.array_equal(top[b, 1:n], recs[b]["top"])
            assert recs[0]["logprobs"].size == 0 and recs[0]["top"].size == 0
        kv, st = _snap(gm, L, max(lens))
        hist = [gm.history(b, n) for b, n in enumerate(lens)]
        for _ in range(6):
            gm.step()
        gm.sync()
        out.append((kv, st, hist, [gm.history(b, n + 6) for b, n in enumerate(lens)]))
    (kv0, st0, h0, c0), (kv1, st1, h1, c1) = out
    assert st0 == st1
    for b in range(4):
        assert all(np.array_equal(x, y) for x, y in zip(kv0[b], kv1[b])), b
        assert np.array_equal(h0[b], h1[b]) and np.array_equal(c0[b], c1[b]), b
    # again, two sequences of other lengths: a 32-row chunk after the 64-row one
    again = [_prompt(n, cfg.vocab_size, seed=21) for n in (9, 14)]
    recs = gm.score(again)
    gm.close()
    _hold(recs, again, _oracle_refs(oracle, name, cfg, again, seed), 0, "case g, second call")


def test_scoring_one_sequence_of_a_running_batch(gpu, oracle):
    """Case g: scoring sequence 2 of a running batch of 4 leaves the other three's rows, state and history as they were."""
    from simplellminference_amd.model import LlamaModel, preset
    from tests.test_gpu_batch_prefill import PROMPTS
    name, _, w, _, seed, _, _ = CASES["b"]
    cfg = preset(name)
    L = cfg.num_hidden_layers
    gm = LlamaModel(config=cfg, w_dtype=w, kv_dtype="f16", seed=seed, batch=4).init()
    gm.predict_batch(PROMPTS, 12)
    kv0, st0 = _snap(gm, L, 64)
    h0 = [gm.history(b, 12) for b in range(4)]
    p_new = _prompt(23, cfg.vocab_size, seed=9)
    recs = gm.score([p_new], seqs=[2])
    kv1, st1 = _snap(gm, L, 64)
    for b in (0, 1, 3):
        assert st1[b] == st0[b]
        assert all(np.array_equal(x, y) for x, y in zip(kv0[b], kv1[b])), b
        assert np.array_equal(gm.history(b, 12), h0[b])
    n = len(p_new)
    assert (st1[2]["pos"], st1[2]["token"], st1[2]["error"]) == (n - 1, p_new[-1], 0)
    assert np.array_equal(gm.history(2, n), p_new)
    gm.close()
    _hold(recs, [p_new], _oracle_refs(oracle, name, cfg, [p_new], seed), 0, "case g, sequence 2")


def test_refusals(gpu):
    """Case h: fp32 weights, an fp32 cache and a rank of an in-process group: score_ok() is false, the call
    SLI_ERR_STATE."""
    from simplellminference_amd._lib import SliError
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    cfg = preset("tiny-gqa")
    for kw in (dict(w_dtype="f16", kv_dtype="f32", batch=2), dict(w_dtype="f32", kv_dtype="f16", batch=1)):
        m = LlamaModel(config=cfg, seed=0, **kw).init()
        assert not m.score_ok()
        with pytest.raises(SliError) as e:
            m.score([[1, 2, 3]])
        assert e.value.code == 7, e.value
        m.close()
    g = TPGroup(preset("tiny-h8"), 2, w_dtype="f16", kv_dtype="f16", seed=0, batch=2).init()
    assert not g.ranks[0].score_ok()
    with pytest.raises(SliError) as e:
        g.ranks[0].score([[1, 2, 3]])
    assert e.value.code == 7 and "vocab-sharded" in str(e.value), e.value
    g.close()


def test_perplexity(gpu):
    """Case i: perplexity(prompts) is exp(-mean) of the returned log-probabilities, to 1e-12 relative."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    prompts = [_prompt(n, cfg.vocab_size) for n in LENS]
    gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=2, batch=4).init()
    recs = gm.score(prompts)
    gm.reset()
    ppl = gm.perplexity(prompts)
    gm.close()
    allp = np.concatenate([r["logprobs"] for r in recs]).astype(np.float64)
    want = float(np.exp(-allp.mean()))
    assert abs(ppl - want) <= 1e-12 * want, (ppl, want)
    assert 1.0 < ppl < 10 * cfg.vocab_size
