"""Continuing sequences from a start position (sli_model_extend_seqs, sli_model_score_extend_seqs, sli_model_extend,
sli_tp_group_extend; LlamaModel.extend / append / score_extend / admit, TPGroup.extend), and the prompt calls as the
start-0 case of them.

Bars: the project's own, from tests/test_gpu_batch_prefill.py and tests/test_gpu_score.py: against the oracle's predict
over each sequence's full forced list greedy tokens bit-equal, logits of every compared position within 1e-3, the K/V
rows a continuation wrote within 2e-3; |d logprob| and |d top_logprob| <= 2e-3, `top` equal wherever the oracle's top-2
gap exceeds 2e-3 with at most 5 % of the positions left out. MXFP4 weights with an FP8 cache are held against the same
model's own teacher-forced decode route under the bars tests/test_gpu_batch_prefill.py quotes for them (logits 1e-3,
argmax where the top-2 gap exceeds 2e-3, the share of differing K/V codes at most tests/kv8_ref.py's FLIP_CAP).

The scenarios and their weight seeds come from tests/extend_scenarios.py (the oracle alone, on the CPU; `python -m
tests.extend_scenarios` prints the scan). Minimum top-2 gap over the compared positions at the recorded seeds: turn 21:
3.0e-3 (seed 0: 1.9e-4); turn, int8: 17: 2.9e-3; rollback 15: 1.2e-2 (sequence 2 from its first decoded position
on); admit 15: 7.3e-3; one-sequence routes 17: 5.9e-3 (fp32 cache 5.9e-3, tiny-h8 1.9e-2); the position edge 0:
2.2e-2; a shorter prompt after a longer one 10: 3.5e-2 (fp32 cache 3.5e-2; tiny-h8 21: 5.3e-2). So the oracle alone
leaves nothing out.
"""
import ctypes

import numpy as np
import pytest

from tests import extend_scenarios as S
from tests import score_ref as R

pytestmark = pytest.mark.gpu

LOGIT, KV, BAR, GAP = 1e-3, 2e-3, 2e-3, 2e-3


def _steps(gm, k, rec=None):
    """k decode steps; rec[b][pos] = the logits of the step that fed sequence b's position pos."""
    for _ in range(k):
        pos = [gm.state(b)["pos"] for b in range(gm.batch)] if rec is not None else None
        gm.step()
        if rec is not None:
            lg = gm.logits()[0].reshape(gm.batch, -1)
            for b in range(gm.batch):
                rec[b][pos[b]] = lg[b].copy()
    gm.sync()


def _kv_all(gm, seq):
    c = gm.config
    return [gm.kv(layer, which, c.max_length, seq=seq) for layer in range(c.num_hidden_layers) for which in (0, 1)]


def _snap(gm, seq):
    return _kv_all(gm, seq), gm.state(seq), gm.history(seq, gm.config.max_length)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1] and np.array_equal(a[2], b[2])


def _hold(tag, hist, rec, otok, olog, first):
    """Tokens over the whole run bit-equal; the recorded logits from position `first` on within the bar."""
    assert np.array_equal(hist, otok[:len(hist)]), (tag, hist, otok)
    got = sorted(p for p in rec if p >= first)
    assert got, tag
    err = max(float(np.abs(rec[p] - olog[p]).max()) for p in got)
    print(f"{tag}: {len(got)} positions from {got[0]}, max|dlogit| {err:.3e}")
    assert err <= LOGIT, (tag, err)


def _hold_kv(tag, gm, seq, rows, lo, hi):
    c = gm.config
    err = 0.0
    for layer in range(c.num_hidden_layers):
        for which in (0, 1):
            err = max(err, float(np.abs(gm.kv(layer, which, hi, seq=seq)[lo:] - rows[which][layer, lo:hi]).max()))
    print(f"{tag}: K/V rows [{lo}, {hi}) max|d| {err:.3e}")
    assert err <= KV, (tag, err)


def _turn_on_gpu(gm, lists, rec=None):
    """Test 3's scenario on the engine, fed from the forced lists: prefill, 6 steps, the turn appended to 1 and 2."""
    prompts = [lists[b][:n] for b, n in enumerate(S.LENS)]
    gm.prefill_batch(prompts)
    _steps(gm, 6, rec)
    return [lists[1][S.LENS[1] + 6:], lists[2][S.LENS[2] + 6:]]


# ---------------------------------------------------------------- 1. a start of 0 is the old call
def test_start_zero_is_prefill_seqs_bit_for_bit(gpu):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    prompts = [S.prompt(n, cfg.vocab_size) for n in S.LENS]
    out = []
    for route in ("prefill_batch", "extend"):
        gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=16, batch=4).init()
        if route == "extend":
            gm.extend(prompts, starts=[0] * 4)
        else:
            gm.prefill_batch(prompts)
        snaps = [_snap(gm, b) for b in range(4)]
        gm.step()
        gm.sync()
        out.append((snaps, gm.logits()[0].copy(), [gm.state(b) for b in range(4)]))
        gm.close()
    (s0, l0, t0), (s1, l1, t1) = out
    for b in range(4):
        assert _same(s0[b], s1[b]), b
        assert s1[b][1]["pos"] == S.LENS[b] - 1
    assert np.array_equal(l0, l1) and t0 == t1


# ---------------------------------------------------------------- 2. split equals whole, bit for bit
@pytest.mark.parametrize("kv_dtype", ["f16", "f8"])
def test_split_prefill_is_bit_identical_at_equal_chunk_size(gpu, kv_dtype):
    """A 33-token prompt at once (32 rows, one 32-row chunk) against 17 + extend from 16 with 17 (groups {0, 16} and
    {16, 16}) and 11 + extend from 10 with 23 (the unaligned first group {10, 6}, then {16, 16}): every call runs a
    32-row chunk, so K/V rows [0, 32) and the next 8 steps' tokens and logits are array_equal. Sequence 1 of a batch of
    2: a sequence offset in every cache address."""
    from simplellminference_amd import ops
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    p = S.prompt(33, cfg.vocab_size)
    plans = {"whole": [(0, 33)], "A": [(0, 17), (16, 17)], "B": [(0, 11), (10, 23)]}
    assert ops.prefill_pack_from([10], [23])[0].tolist() == [[0, 10, 6], [0, 16, 16]]
    for calls in plans.values():
        for start, count in calls:
            assert ops.prefill_pack_from([start], [count])[1].tolist() == [32]
    out = {}
    for name, calls in plans.items():
        gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype=kv_dtype, seed=16, batch=2).init()
        for start, count in calls:
            gm.extend([p[start:start + count]], seqs=[1], starts=[start])
        assert gm.state(1)["pos"] == 32 and gm.state(1)["token"] == p[32]
        rows = [gm.kv(layer, which, 32, seq=1) for layer in range(cfg.num_hidden_layers) for which in (0, 1)]
        rec = [{}, {}]
        _steps(gm, 8, rec)
        out[name] = (rows, gm.history(1, 41), np.stack([rec[1][t] for t in range(32, 40)]))
        gm.close()
    for name in ("A", "B"):
        for x, y in zip(out["whole"][0], out[name][0]):
            assert np.array_equal(x, y), name
        assert np.array_equal(out["whole"][1], out[name][1]), name
        assert np.array_equal(out["whole"][2], out[name][2]), name


# ---------------------------------------------------------------- 3. a second turn against the oracle
@pytest.mark.parametrize("w,scen", [("f16", "turn"), ("i8", "turn-i8")])
def test_second_turn_matches_oracle(gpu, oracle, w, scen):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    seed = S.SEEDS[scen]
    kw = dict(wmode=oracle.W_I8) if w == "i8" else {}
    lists, first = S.turn(oracle, cfg, seed, **kw)
    gm = LlamaModel(config=cfg, w_dtype=w, kv_dtype="f16", seed=seed, batch=4).init()
    rec = [{} for _ in range(4)]
    turns = _turn_on_gpu(gm, lists, rec)
    before = {b: _snap(gm, b) for b in (0, 3)}
    pos0 = [gm.state(b)["pos"] for b in range(4)]
    gm.append(turns, seqs=[1, 2])
    for b in (0, 3):
        assert _same(before[b], _snap(gm, b)), b
    for b, t in zip((1, 2), turns):
        st = gm.state(b)
        assert (st["pos"], st["token"], st["error"]) == (pos0[b] + len(t), t[-1], 0)
        assert np.array_equal(gm.history(b, st["pos"] + 1), lists[b])
    _steps(gm, 63 - min(gm.state(b)["pos"] for b in range(4)) + 1, rec)
    for b in range(4):
        otok, olog, rows = S.run(oracle, cfg, lists[b], 64, seed, kv=True, **kw)
        assert gm.state(b)["pos"] == 63
        _hold(f"{scen} sequence {b}", gm.history(b, 64), rec[b], otok, olog, first[b])
        if b in (1, 2):  # the rows the turn wrote: from the pending token's position to the last appended one's - 1
            _hold_kv(f"{scen} sequence {b}", gm, b, rows, pos0[b], len(lists[b]) - 1)
    gm.close()


def test_second_turn_mxfp4_fp8_cache_against_own_decode_route(gpu):
    """The turn on MXFP4 weights (mx_batch) with an FP8 cache, against the same model's own teacher-forced decode route
    over the tokens the run fed (predict_batch with the whole history forced): logits within 1e-3, argmax equal where
    the decode route's top-2 gap exceeds 2e-3, at most FLIP_CAP of the K/V codes of the extended rows differ."""
    from tests import kv8_ref as K8
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    make = lambda: LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f8", seed=7, batch=4, mx_batch=True).init()
    prompts = [S.prompt(n, cfg.vocab_size) for n in S.LENS]
    turns = [S.prompt(3, cfg.vocab_size, seed=99), S.prompt(20, cfg.vocab_size, seed=99)]
    gm = make()
    rec = [{} for _ in range(4)]
    gm.prefill_batch(prompts)
    _steps(gm, 6, rec)
    pos0 = [gm.state(b)["pos"] for b in range(4)]
    gm.append(turns, seqs=[1, 2])
    _steps(gm, 63 - min(gm.state(b)["pos"] for b in range(4)) + 1, rec)
    hist = [gm.history(b, 64).tolist() for b in range(4)]
    rows = [_kv_all(gm, b) for b in range(4)]
    gm.close()
    own = make()
    _, ologits = own.predict_batch(hist, 64, want_logits=True)
    orows = [_kv_all(own, b) for b in range(4)]
    own.close()
    flips = compared = 0
    for b, t in zip((1, 2), turns):
        lo, hi = pos0[b], pos0[b] + len(t)
        for x, y in zip(rows[b], orows[b]):
            flips += int((K8.encode(x[lo:hi]) != K8.encode(y[lo:hi])).sum())
            compared += x[lo:hi].size
    print(f"{flips} of {compared} K/V codes of the extended rows differ")
    assert compared > 0 and flips <= K8.FLIP_CAP * compared, (flips, compared)
    for b in range(4):
        ps = sorted(rec[b])
        got, ref = np.stack([rec[b][p] for p in ps]), ologits[b, ps]
        err = float(np.abs(got - ref).max())
        print(f"sequence {b}: {len(ps)} positions, max|dlogit| {err:.3e}")
        assert err <= LOGIT, (b, err)
        s = np.sort(ref, axis=-1)
        clear = (s[:, -1] - s[:, -2]) > GAP
        assert np.array_equal(np.argmax(got, -1)[clear], np.argmax(ref, -1)[clear]), b


# ---------------------------------------------------------------- 4. rollback
def test_rollback_matches_oracle(gpu, oracle):
    """After the turn sequence 2 stands at 42; it goes back to 20 with 9 other tokens: rows 20 .. 27 are overwritten,
    the stale rows behind them are never read."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    seed = S.SEEDS["rollback"]
    lists, _ = S.turn(oracle, cfg, seed)
    (forced,), _ = S.rollback(oracle, cfg, seed)
    gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=seed, batch=4).init()
    gm.append(_turn_on_gpu(gm, lists), seqs=[1, 2])
    assert gm.state(2)["pos"] == 42
    others = {b: _snap(gm, b) for b in (0, 1, 3)}
    gm.extend([forced[20:]], seqs=[2], starts=[20])
    assert gm.state(2)["pos"] == 28 and np.array_equal(gm.history(2, 29), forced)
    for b in (0, 1, 3):
        assert _same(others[b], _snap(gm, b)), b
    rec = [{} for _ in range(4)]
    _steps(gm, 36, rec)
    otok, olog, rows = S.run(oracle, cfg, forced, 64, seed, kv=True)
    _hold("rollback", gm.history(2, 64), rec[2], otok, olog, 28)
    _hold_kv("rollback", gm, 2, rows, 20, 28)
    gm.close()


# ---------------------------------------------------------------- 5. chunked admission
def test_chunked_admission_matches_oracle(gpu, oracle):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa", max_length=320)
    seed = S.SEEDS["admit"]
    ps, first = S.admit(oracle, cfg, seed)
    gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=seed, batch=4).init()
    rec = [{} for _ in range(4)]
    gm.prefill_batch(ps[:3], seqs=[0, 1, 2])
    calls, waits = [], []

    def between():
        calls.append(gm.state(3)["pos"])
        _steps(gm, 2, rec)
        waits.append(gm.state(3)["pos"])

    gm.admit([ps[3]], [3], max_tokens=100, between=between)
    # calls over tokens [0, 97), [96, 193), [192, 289), [288, 300) (each at most 100, every call but the last ending one
    # past a 16-boundary): sequence 3 waits at 96, 192, 288 and does not move while the others step
    assert calls == [96, 192, 288] and waits == calls
    assert S.ADMIT_BETWEEN == 2 * len(calls)
    st = gm.state(3)
    assert (st["pos"], st["token"]) == (299, ps[3][-1])
    rec[3] = {}  # the waiting steps' logits are not the run's
    _steps(gm, S.ADMIT_AFTER, rec)
    for b in range(4):
        steps = len(ps[b]) + S.ADMIT_AFTER + (S.ADMIT_BETWEEN if b < 3 else 0)
        otok, olog, rows = S.run(oracle, cfg, ps[b], steps, seed, kv=b == 3)
        assert gm.state(b)["pos"] == steps - 1
        _hold(f"admit sequence {b}", gm.history(b, steps), rec[b], otok, olog, first[b])
        if b == 3:
            _hold_kv("admit sequence 3", gm, 3, rows, 0, 299)
    gm.close()


# ---------------------------------------------------------------- 6. scoring from a start
def _raw_score_extend(gm, tokens, seqs, starts):
    from simplellminference_amd._lib import call
    P, counts, ld = gm._ragged(tokens)
    seqs, starts = np.asarray(seqs, np.int32), np.asarray(starts, np.int32)
    lp, top, tlp = np.zeros(P.shape, np.float32), np.zeros(P.shape, np.int32), np.zeros(P.shape, np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call("sli_model_score_extend_seqs", gm._h, vp(seqs), seqs.size, vp(P), vp(starts), vp(counts), ld, 1, vp(lp),
         vp(top), vp(tlp))
    return lp, top, tlp, counts


def test_score_extend_matches_score_ref_and_leaves_what_extend_leaves(gpu, oracle):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    seed = S.SEEDS["turn"]
    lists, _ = S.turn(oracle, cfg, seed)
    out = []
    for route in ("extend", "score"):
        gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=seed, batch=4).init()
        assert gm.score_ok()
        turns = _turn_on_gpu(gm, lists)
        pos0 = [gm.state(b)["pos"] for b in range(4)]
        toks = [[lists[b][pos0[b]], *t] for b, t in zip((1, 2), turns)]
        if route == "extend":
            gm.extend(toks, seqs=[1, 2])
            res = None
        else:
            res = _raw_score_extend(gm, toks, [1, 2], [pos0[1], pos0[2]])
        snaps = [_snap(gm, b) for b in range(4)]
        gm.step()
        gm.sync()
        out.append((snaps, gm.logits()[0].copy(), res, pos0, toks))
        gm.close()
    (s0, l0, _, _, _), (s1, l1, (lp, top, tlp, counts), pos0, toks) = out
    for b in range(4):
        assert _same(s0[b], s1[b]), b
    assert np.array_equal(l0, l1)
    left = total = 0
    for i, b in enumerate((1, 2)):
        n = int(counts[i])
        assert np.isnan(lp[i, 0]) and top[i, 0] == -1 and np.isnan(tlp[i, 0])
        assert np.isnan(lp[i, n:]).all() and (top[i, n:] == -1).all() and np.isnan(tlp[i, n:]).all()
        _, olog, _ = S.run(oracle, cfg, lists[b], len(lists[b]), seed)
        rows = olog[pos0[b]:pos0[b] + n - 1]  # position start + j - 1 scores tokens[j]
        rlp, rtop, rtlp = R.score_rows(rows, toks[i][1:])
        gap = np.array([R.top2_gap(r) for r in rows])
        e1, e2 = float(np.abs(lp[i, 1:n] - rlp).max()), float(np.abs(tlp[i, 1:n] - rtlp).max())
        print(f"sequence {b}: max|d logprob| {e1:.3e}, max|d top_logprob| {e2:.3e}")
        assert e1 <= BAR and e2 <= BAR, (b, e1, e2)
        clear = gap > GAP
        assert np.array_equal(top[i, 1:n][clear], rtop[clear]), b
        left += int((~clear).sum())
        total += n - 1
    assert left <= 0.05 * total, (left, total)


def test_score_extend_records(gpu):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=0, batch=2).init()
    gm.prefill_batch([S.prompt(20, cfg.vocab_size)], seqs=[1])
    recs = gm.score_extend([[gm.state(1)["token"], 5, 6, 7]], seqs=[1])
    assert [r.shape for r in recs[0].values()] == [(3,)] * 3 and np.isfinite(recs[0]["logprobs"]).all()
    assert gm.state(1)["pos"] == 22
    gm.close()


# ---------------------------------------------------------------- 7. the one-sequence routes
@pytest.mark.parametrize("route", ["gemm", "decode", "f32kv", "tp2"])
def test_one_sequence_routes_match_oracle(gpu, oracle, route):
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    scen = {"f32kv": "one-f32kv", "tp2": "one-tp"}.get(route, "one")
    cfg = preset("tiny-h8" if route == "tp2" else "tiny-gqa")
    seed = S.SEEDS[scen]
    okw = dict(kv_f16=False) if route == "f32kv" else {}
    (forced,), (first,) = S.one(oracle, cfg, seed, **okw)
    if route == "tp2":
        gm = TPGroup(cfg, 2, w_dtype="f16", kv_dtype="f16", seed=seed).init()
        state, hist, extend = gm.ranks[0].state, gm.ranks[0].history, gm.extend
        logits = gm.logits
    else:
        gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f32" if route == "f32kv" else "f16", seed=seed).init()
        state, hist, extend = gm.state, gm.history, gm.extend_one
        logits = lambda: gm.logits()[0]
        if route != "f32kv":
            gm.set_prefill(route)
        assert gm.prefill_path() == ("decode" if route == "decode" else "mfma")
    rec = {}

    def steps(k):
        for _ in range(k):
            p = state()["pos"]
            gm.step()
            rec[p] = np.array(logits()).reshape(-1).copy()
        gm.sync()

    gm.prefill(forced[:20])
    steps(3)
    assert state()["pos"] == 22 and state()["token"] == forced[22]
    extend(forced[22:])  # the pending token, then the turn: from the current position
    assert (state()["pos"], state()["token"]) == (len(forced) - 1, forced[-1])
    steps(64 - len(forced) + 1)
    otok, olog, rows = S.run(oracle, cfg, forced, 64, seed, kv=route != "tp2", **okw)
    _hold(f"one-sequence {route}", hist(0, 64), rec, otok, olog, first)
    if route != "tp2":
        _hold_kv(f"one-sequence {route}", gm, 0, rows, 22, len(forced) - 1)
    gm.close()


def test_one_sequence_extend_from_a_given_start(gpu, oracle):
    """start given (a rollback on the one-sequence route) on the GEMM path and the decode path: the same oracle run."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    seed = S.SEEDS["one"]
    (forced,), _ = S.one(oracle, cfg, seed)
    otok, _, _ = S.run(oracle, cfg, forced, 48, seed)
    for mode in ("gemm", "decode"):
        gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=seed).init()
        gm.set_prefill(mode)
        gm.prefill(S.prompt(30, cfg.vocab_size, seed=4))  # another prompt first: rows 0 .. 28 are overwritten below
        gm.extend_one(forced[:11], start=0)
        gm.extend_one(forced[10:], start=10)
        for _ in range(48 - len(forced) + 1):
            gm.step()
        gm.sync()
        assert np.array_equal(gm.history(0, 48), otok), mode
        gm.close()


# ---------------------------------------------------------------- 8. the position edge
def test_position_edge_matches_oracle(gpu, oracle):
    """max_length 40. Sequence 0: start 35, count 4: the partial first group {35, 3} has padding rows at positions 38 ..
    50, past max_len - 1. Sequence 1: start 19, count 21: start + count == max_len."""
    from simplellminference_amd import ops
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa", max_length=40)
    seed = S.SEEDS["edge"]
    lists, first = S.edge(oracle, cfg, seed)
    assert ops.prefill_pack_from([35], [4])[0].tolist() == [[0, 35, 3], [0, 0, 0]]
    gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=seed, batch=3).init()
    gm.prefill_batch([lists[0][:36], lists[1][:20], S.prompt(25, cfg.vocab_size, seed=8)])
    for b, start in ((0, 35), (1, 19)):
        others = {o: _snap(gm, o) for o in range(3) if o != b}
        gm.extend([lists[b][start:]], seqs=[b], starts=[start])
        for o, s in others.items():
            assert _same(s, _snap(gm, o)), (b, o)
    assert gm.state(0)["pos"] == 38 and gm.state(1)["pos"] == 39
    rec = [{} for _ in range(3)]
    _steps(gm, 2, rec)
    for b in (0, 1):
        otok, olog, rows = S.run(oracle, cfg, lists[b], 40, seed, kv=True)
        _hold(f"edge sequence {b}", gm.history(b, 40), rec[b], otok, olog, first[b])
        _hold_kv(f"edge sequence {b}", gm, b, rows, first[b], len(lists[b]) - 1)
    gm.close()


# ---------------------------------------------------------------- 10. refusals
def _raw_extend(m, tokens, seqs, starts):
    from simplellminference_amd._lib import call
    P, counts, ld = m._ragged(tokens)
    seqs, starts = np.asarray(seqs, np.int32), np.asarray(starts, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call("sli_model_extend_seqs", m._h, vp(seqs), seqs.size, vp(P), vp(starts), vp(counts), ld, 1)


def test_refusals_leave_every_state_as_it_was(gpu):
    from simplellminference_amd._lib import SliError
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    cfg = preset("tiny-gqa")
    gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=0, batch=4).init()
    gm.prefill_batch([S.prompt(n, cfg.vocab_size) for n in (5, 9, 3, 12)])
    _steps(gm, 3)
    before = [_snap(gm, b) for b in range(4)]

    def refused(code, fn, *a, **k):
        with pytest.raises(SliError) as e:
            fn(*a, **k)
        assert e.value.code == code, e.value

    refused(1, gm.extend, [[1, 2], [3, 4]], seqs=[1, 1])                     # SLI_ERR_ARG: a duplicate
    refused(1, gm.extend, [[1, 2]], seqs=[4])
    refused(3, gm.extend, [[1, 2], []], seqs=[0, 1])                         # SLI_ERR_RANGE: count 0
    refused(3, gm.extend, [[1] * 60], seqs=[0])                              # 7 + 60 > 64
    refused(3, gm.extend, [[1, cfg.vocab_size]], seqs=[0])                   # a token outside the vocabulary
    refused(3, gm.extend, [[1, 2]], seqs=[0], starts=[8])                    # a start above the position (7)
    refused(3, gm.extend, [[1, 2]], seqs=[0], starts=[-1])
    refused(3, gm.score_extend, [[1, 2]], seqs=[0], starts=[8])
    refused(1, gm.fork, 1, 1, 2)                                             # src == dst
    refused(3, gm.fork, 0, 1, 8)                                             # n above src's position
    refused(3, gm.fork, 0, 1, -1)
    assert all(_same(x, _snap(gm, b)) for b, x in enumerate(before))
    gm.close()
    # the SLI_ERR_STATE reasons of prefill_seqs: an fp32 cache, fp32 weights, a group rank; scoring under TP
    for kw in (dict(w_dtype="f16", kv_dtype="f32", batch=2), dict(w_dtype="f32", kv_dtype="f16", batch=1)):
        m = LlamaModel(config=cfg, seed=0, **kw).init()
        st = m.state(0)
        for fn in (m.extend, m.score_extend):
            with pytest.raises(SliError) as e:
                fn([[1, 2, 3]], seqs=[0], starts=[0])
            assert e.value.code == 7 and ("fp32" in str(e.value)), e.value
        assert m.state(0) == st
        m.close()
    g = TPGroup(preset("tiny-h8"), 2, w_dtype="f16", kv_dtype="f16", seed=0, batch=2).init()
    for fn in (g.ranks[0].extend, g.ranks[0].score_extend):
        with pytest.raises(SliError) as e:
            fn([[1, 2, 3]], seqs=[0], starts=[0])
        assert e.value.code == 7 and "group" in str(e.value), e.value
    g.close()


# ---------------------------------------------------------------- 11. a prompt is a continuation from 0
def _one_sequence_engine(route, seed):
    """A fresh batch-1 engine on `route`: (engine, its rank models, its one-sequence extend, the oracle's keywords)."""
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    if route == "tp2":
        g = TPGroup(preset("tiny-h8"), 2, w_dtype="f16", kv_dtype="f16", seed=seed).init()
        assert g.prefill_path() == "mfma"
        return g, g.ranks, g.extend, {}
    kv = "f32" if route == "f32kv" else "f16"
    gm = LlamaModel(config=preset("tiny-gqa"), w_dtype="f16", kv_dtype=kv, seed=seed).init()
    if route != "f32kv":
        gm.set_prefill(route)
    assert gm.prefill_path() == ("decode" if route == "decode" else "mfma")
    return gm, [gm], gm.extend_one, dict(kv_f16=False) if route == "f32kv" else {}


@pytest.mark.parametrize("route", ["gemm", "decode", "f32kv", "tp2"])
def test_prefill_is_extend_from_zero_on_the_one_sequence_routes(gpu, route):
    """37 tokens: positions 0 .. 35 are prefilled, two full groups and a partial one in the 64-row bucket. prefill()
    against the one-sequence extend from start 0 on two fresh engines, then one step of each: per rank the state behind
    the call and, behind the step, K/V rows [0, 37), the state, history [0, 38) and the logits are array_equal."""
    out = []
    for call in ("prefill", "extend"):
        gm, ranks, extend, _ = _one_sequence_engine(route, 16)
        p = S.prompt(37, gm.config.vocab_size)
        if call == "prefill":
            gm.prefill(p)
        else:
            extend(p, start=0)
        left = [m.state() for m in ranks]
        assert all((st["pos"], st["token"], st["error"]) == (36, p[36], 0) for st in left)
        gm.step()
        gm.sync()
        layers = range(gm.config.num_hidden_layers)
        out.append([(left[r], [m.kv(layer, which, 37) for layer in layers for which in (0, 1)], m.state(),
                     m.history(0, 38), m.logits()[0].copy()) for r, m in enumerate(ranks)])
        gm.close()
    for r, (a, b) in enumerate(zip(*out)):
        assert a[0] == b[0] and a[2] == b[2], (route, r, a[0], b[0], a[2], b[2])
        assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1])), (route, r)
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), (route, r)
        assert a[2]["pos"] == 37


@pytest.mark.parametrize("route", ["decode", "f32kv", "tp2"])
def test_shorter_prompt_after_a_longer_one_without_reset(gpu, oracle, route):
    """predict_prefill of a 40-token prompt to 46, then on the same engine of a 9-token prompt to 15 (nothing reset in
    between: the first call's longer forced prefix, its advancing state and its rows 8 .. 45 are still there): each
    call's tokens equal the oracle's predict, its logits from the last prompt position on are within the bar, and the
    engine stands where a fresh one stands after the second call alone. (The GEMM route of a single model:
    tests/test_gpu_prefill.py::test_prefill_twice_reuses_graphs.)"""
    seed = S.SEEDS[{"decode": "again", "f32kv": "again-f32kv", "tp2": "again-tp"}[route]]
    gm, ranks, _, okw = _one_sequence_engine(route, seed)
    cfg = gm.config
    for n, upto in S.AGAIN:
        p = S.prompt(n, cfg.vocab_size)
        toks, logits = gm.predict_prefill(p, upto, want_logits=True)
        otok, olog, _ = S.run(oracle, cfg, p, upto, seed, **okw)
        assert np.array_equal(toks, otok), (route, n, toks, otok)
        assert np.isnan(logits[:n - 1]).all()
        err = float(np.abs(logits[n - 1:] - olog[n - 1:]).max())
        print(f"{route}, prompt of {n} to {upto}: max|dlogit| {err:.3e}")
        assert err <= LOGIT, (route, n, err)
    fresh, franks, _, _ = _one_sequence_engine(route, seed)
    n, upto = S.AGAIN[1]
    ftoks = fresh.predict_prefill(S.prompt(n, cfg.vocab_size), upto)
    assert np.array_equal(toks, ftoks)
    for m, f in zip(ranks, franks):
        assert m.state()["error"] == 0 and m.state()["pos"] == f.state()["pos"] == upto, (m.state(), f.state())
    gm.close()
    fresh.close()
