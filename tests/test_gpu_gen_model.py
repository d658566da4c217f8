"""Per-sequence generation inside the engine's step (sli.h at sli_model_set_gen_seq): every sequence of a batch with a
block of its own, judged by tests/gen_ref.py against the GPU's own logits of the step before and the tokens the run
itself produced (the method of tests/test_gpu_sample.py); the graphs; the stop rule; the refusals and range errors."""
import numpy as np
import pytest

from tests import gen_ref as G
from tests import sample_ref as R

pytestmark = pytest.mark.gpu

STEPS = 36
PROMPTS = [[5, 17, 300, 42, 9], [511], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [77, 78]]
MODELS = [("tiny", 1, "f16", "f16"), ("tiny-gqa", 4, "f16", "f16"), ("tiny", 1, "i8", "f8"),
          ("tiny-gqa", 4, "i8", "f8")]


def _blocks(prompts):
    """Four different blocks: greedy; sampled; sampled with min-p and all three penalties over the generated tokens
    only; greedy with penalties over everything."""
    return [G.params(),
            G.params(temperature=0.05, top_k=40, top_p=0.9, seed=21),
            G.params(temperature=0.05, seed=22, min_p=0.1, repetition_penalty=1.3, presence_penalty=0.02,
                     frequency_penalty=0.01, penalty_from=len(prompts[min(2, len(prompts) - 1)])),
            G.params(temperature=0.0, repetition_penalty=1.2, presence_penalty=0.01)]


def _model(name, B, w, kv, seed=3, **over):
    from simplellminference_amd.model import LlamaModel, preset
    return LlamaModel(config=preset(name, **over), w_dtype=w, kv_dtype=kv, seed=seed, batch=B).init()


def _run(m, B, prompts):
    """tokens [B, STEPS], logits [B, STEPS, V]"""
    if B == 1:
        toks, logits = m.predict(prompts[0], STEPS, want_logits=True)
        return toks[None], logits[None]
    return m.predict_batch(prompts, STEPS, want_logits=True)


def _check_run(m, toks, logits, prompts, blocks):
    for b, (prompt, P) in enumerate(zip(prompts, blocks)):
        assert toks[b, :len(prompt)].tolist() == prompt
        for t in range(len(prompt) - 1, STEPS - 1):
            ok, why = G.accept(toks[b, t + 1], logits[b, t], toks[b], t, P, b)
            assert ok, ("sequence", b, "position", t, why)
        # the state after the last step: the token chosen from the last logits was fed; last_argmax stays the raw argmax
        hist = m.history(b, STEPS + 1)
        assert np.array_equal(hist[:STEPS], toks[b]) and m.sampled(b) == hist[STEPS] == m.state(b)["token"]
        ok, why = G.accept(hist[STEPS], logits[b, STEPS - 1], hist, STEPS - 1, P, b)
        assert ok, why
        assert m.state(b)["last_argmax"] == R.argmax_a8(logits[b, STEPS - 1])


@pytest.mark.parametrize("name,B,w,kv", MODELS)
def test_every_sequence_with_its_own_block(gpu, name, B, w, kv):
    prompts = PROMPTS[:B]
    m = _model(name, B, w, kv)
    greedy_toks, greedy_logits = _run(m, B, prompts)
    assert m.finished().tolist() == [0] * B and m.generation(0)["temperature"] == 0.0
    blocks = _blocks(prompts)
    # batch 4: the four blocks side by side; batch 1: one after the other
    for rot in range(1 if B > 1 else 4):
        use = [blocks[(b + rot) % 4] for b in range(B)]
        for b, P in enumerate(use):
            m.set_generation(b, **P)
            got = m.generation(b)
            assert got["seed"] == P["seed"] and got["penalty_from"] == P["penalty_from"] and got["stop"] == ()
            assert got["min_p"] == np.float32(P["min_p"])
        toks, logits = _run(m, B, prompts)
        _check_run(m, toks, logits, prompts, use)
        for b, P in enumerate(use):
            if P == blocks[0]:  # the greedy sequence: the greedy run's tokens and logits, bit for bit
                assert np.array_equal(toks[b], greedy_toks[b])
                assert np.array_equal(logits[b].view(np.uint32), greedy_logits[b].view(np.uint32))
            elif P["temperature"] != 0.0:
                assert not np.array_equal(toks[b], greedy_toks[b])
        toks2, logits2 = _run(m, B, prompts)  # the same blocks: the same run
        assert np.array_equal(toks2, toks) and np.array_equal(logits2.view(np.uint32), logits.view(np.uint32))
    assert m.finished().tolist() == [0] * B  # no stop set, and the last position was not reached
    m.close()


def test_graphs(gpu):
    B, prompts = 4, PROMPTS
    m = _model("tiny-gqa", B, "f16", "f16")
    greedy_toks, greedy_logits = _run(m, B, prompts)
    assert m.graph_captures() == 1
    blocks = _blocks(prompts)
    m.set_generation(1, **blocks[1])  # entering the mode: one capture
    toks, logits = _run(m, B, prompts)
    assert m.graph_captures() == 2
    _check_run(m, toks, logits, prompts, [blocks[0], blocks[1], blocks[0], blocks[0]])
    for b in range(B):  # any block changes: none
        m.set_generation(b, **blocks[(b + 2) % 4])
    m.set_generation(0, None)
    m.set_generation(3, max_pos=50, **blocks[1])
    toks, logits = _run(m, B, prompts)
    assert m.graph_captures() == 2
    _check_run(m, toks, logits, prompts, [blocks[0], blocks[3], blocks[0], blocks[1]])
    # set_sampling(None) leaves the mode: the greedy run in token and logit bits, one capture, every block cleared
    m.set_sampling(None)
    assert m.generation(3)["stop"] == () and m.generation(1)["repetition_penalty"] == 1.0
    again_toks, again_logits = _run(m, B, prompts)
    assert m.graph_captures() == 3 and m.sampled() == -1
    assert np.array_equal(again_toks, greedy_toks)
    assert np.array_equal(again_logits.view(np.uint32), greedy_logits.view(np.uint32))
    # the model-level sampler afterwards: as tests/test_gpu_sample.py expects it
    m.set_generation(2, **blocks[2])
    T, k, p = 0.05, 40, 0.9
    m.set_sampling(T, top_k=k, top_p=p, seed=21)
    assert m.generation(2)["repetition_penalty"] == 1.0 and m.sampling()["top_k"] == k
    s_toks, s_logits = _run(m, B, prompts)
    for b, prompt in enumerate(prompts):
        assert s_toks[b, :len(prompt)].tolist() == prompt
        for t in range(len(prompt) - 1, STEPS - 1):
            ok, why = R.accept(s_toks[b, t + 1], s_logits[b, t], T, k, p, 21, b, t)
            assert ok, ("sequence", b, "position", t, why)
    # and the same block per sequence draws the same tokens as the model-level setting
    for b in range(B):
        m.set_generation(b, temperature=T, top_k=k, top_p=p, seed=21)
    assert m.sampling() is None
    g_toks, g_logits = _run(m, B, prompts)
    assert np.array_equal(g_toks, s_toks) and np.array_equal(g_logits.view(np.uint32), s_logits.view(np.uint32))
    m.close()


def _start(m, prompts):
    m.reset()
    for b, p in enumerate(prompts):
        m.set_prompt_seq(b, p)
        m.set_state_seq(b, p[0], 0, advance=True)


def test_stop_rule(gpu):
    B, prompts = 4, PROMPTS
    m = _model("tiny-gqa", B, "f16", "f16")
    T = m.config.max_length
    greedy = m.predict_batch(prompts, STEPS)
    # sequence 1 stops at the first occurrence of its 6th generated token; sequence 0's stop token stands in its
    # prompt and is never generated; sequence 2 may reach position 20; sequence 3 has no condition
    s1 = int(greedy[1, len(prompts[1]) + 5])
    p1 = int(np.flatnonzero(greedy[1, len(prompts[1]):] == s1)[0]) + len(prompts[1])
    s0 = [t for t in prompts[0] if t not in greedy[0, len(prompts[0]):]][0]
    m.set_generation(0, stop=(s0,))
    m.set_generation(1, stop=(499, s1))
    m.set_generation(2, max_pos=20)
    m.set_generation(3)
    _start(m, prompts)
    n_steps = 30
    parked_kv = None
    for step in range(1, n_steps + 1):  # after `step` steps an advancing sequence stands at position `step`
        m.step()
        fin = m.finished()
        assert fin[0] == 0 and fin[3] == 0
        assert fin[1] == (1 if step >= p1 else 0), step
        assert fin[2] == (2 if step >= 20 else 0), step
        st = [m.state(b) for b in range(B)]
        assert st[0]["pos"] == step and st[3]["pos"] == step
        assert (st[1]["pos"], st[1]["token"]) == ((p1, s1) if step >= p1 else (step, greedy[1, step]))
        assert (st[2]["pos"], st[2]["token"]) == ((20, greedy[2, 20]) if step >= 20 else (step, greedy[2, step]))
        if step == p1 + 1:  # one idle step behind the stop: its pending row has been written once
            parked_kv = [m.kv(l, w, p1 + 1, seq=1) for l in range(2) for w in range(2)]
    assert parked_kv is not None and p1 + 1 < n_steps
    for b in (0, 3):  # the others went on, greedily
        assert np.array_equal(m.history(b, n_steps + 1), greedy[b, :n_steps + 1])
    assert np.array_equal(m.history(1, p1 + 1), greedy[1, :p1 + 1])  # the stop token stays in the history
    assert np.array_equal(m.history(2, 21), greedy[2, :21])
    for a, b in zip(parked_kv, [m.kv(l, w, p1 + 1, seq=1) for l in range(2) for w in range(2)]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # host calls that write a sequence's state clear its flag
    m.set_state_seq(1, 7, 3, advance=False)
    assert m.finished().tolist() == [0, 0, 2, 0]
    m.prefill_batch([prompts[2]], [2])
    assert m.finished().tolist() == [0, 0, 0, 0]
    # a waiting sequence is never examined: sequence 1 waits on one of its stop tokens, sequence 0 at the last position
    m.set_state_seq(1, s1, 5, advance=False)
    m.set_state_seq(0, 9, T - 1, advance=False)
    # reaching the last position: length
    m.set_state_seq(3, 9, T - 2, advance=True)
    m.step()
    m.step()
    assert m.finished().tolist() == [0, 0, 0, 2]
    assert m.state(3)["pos"] == T - 1 and m.state(1)["pos"] == 5 and m.state(0)["pos"] == T - 1
    # set_generation for a sequence clears its flag; reset clears all
    m.set_generation(3, None)
    assert m.finished().tolist() == [0, 0, 0, 0]
    m.close()


def test_stop_rule_batch_one_after_prefill(gpu):
    m = _model("tiny", 1, "i8", "f8")
    prompt = PROMPTS[2]
    greedy = m.predict(prompt, STEPS)
    s = int(greedy[len(prompt) + 3])
    p = int(np.flatnonzero(greedy[len(prompt):] == s)[0]) + len(prompt)
    m.set_generation(0, stop=(s,), max_pos=len(prompt) + 10)
    toks = m.predict_prefill(prompt, STEPS)  # a fixed number of steps: the sequence parks inside it
    assert m.finished().tolist() == [1] and m.state()["pos"] == p and m.state()["token"] == s
    assert np.array_equal(toks[:p + 1], greedy[:p + 1])
    m.set_generation(0, max_pos=len(prompt) + 10)
    m.predict_prefill(prompt, STEPS)
    assert m.finished().tolist() == [2] and m.state()["pos"] == len(prompt) + 10
    m.reset()
    assert m.finished().tolist() == [0]
    m.close()


def test_refusals(gpu):
    from simplellminference_amd import SliError
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    g = TPGroup(preset("tiny"), 2, seed=1).init()
    with pytest.raises(SliError, match="in-process tp group") as e:
        g.ranks[1].set_generation(0, 1.0)
    assert e.value.code == 7
    g.close()
    # the persistent layers, in either order of the two setters
    m = LlamaModel(config=preset("small-h128"), w_dtype="f16", kv_dtype="f16", seed=1).init()
    m.set_exec("persist")
    with pytest.raises(SliError, match="persistent layers") as e:
        m.set_generation(0, 1.0)
    assert e.value.code == 7 and m.generation(0)["temperature"] == 0.0
    m.set_exec("launches")
    m.set_generation(0, 1.0, top_k=5)
    with pytest.raises(SliError, match="sampling is on") as e:
        m.set_exec("persist")
    assert e.value.code == 7 and m.exec_mode() == "launches"
    toks = m.predict([1, 2, 3], 8)
    assert toks[:3].tolist() == [1, 2, 3]
    m.close()


def test_range_and_argument_errors(gpu):
    from simplellminference_amd import SliError
    m = _model("tiny-gqa", 2, "f16", "f16")
    V, T = m.config.vocab_size, m.config.max_length
    for kw, code in ((dict(stop=(3, V)), 3), (dict(stop=(-1,)), 3), (dict(max_pos=T), 3), (dict(seq=2), 3),
                     (dict(seq=-1), 3), (dict(temperature=-1.0), 1), (dict(temperature=float("nan")), 1),
                     (dict(min_p=1.0), 1), (dict(repetition_penalty=0.0), 1), (dict(penalty_from=-1), 1)):
        kw = dict(kw)
        with pytest.raises(SliError) as e:
            m.set_generation(kw.pop("seq", 0), **kw)
        assert e.value.code == code, kw
    with pytest.raises(ValueError):
        m.set_generation(0, stop=tuple(range(9)))
    # nothing was written: the model is not in the mode
    assert m.graph_captures() == 0 and m.generation(0)["stop"] == () and m.finished().tolist() == [0, 0]
    m.set_generation(1, stop=(V - 1,), max_pos=T - 1)
    assert m.generation(1)["stop"] == (V - 1,) and m.generation(1)["max_pos"] == T - 1
    m.close()
    # beyond the penalised sampler's capacity: a penalised block is refused with the numbers, every other block runs
    big = _model("tiny", 1, "f16", "f16", max_length=4097)
    with pytest.raises(SliError, match="4097") as e:
        big.set_generation(0, 1.0, presence_penalty=0.5)
    assert e.value.code == 2 and big.graph_captures() == 0
    greedy = big.predict(PROMPTS[0], 12)
    big.set_generation(0, 0.05, top_k=40, seed=3, min_p=0.05, stop=(int(greedy[8]),))
    toks, logits = big.predict(PROMPTS[0], 12, want_logits=True)
    P = G.params(temperature=0.05, top_k=40, seed=3, min_p=0.05)
    for t in range(len(PROMPTS[0]) - 1, min(int(big.state()["pos"]), 11)):  # up to where it parked, if it did
        ok, why = G.accept(toks[t + 1], logits[t], toks, t, P, 0)
        assert ok, (t, why)
    with pytest.raises(SliError) as e:
        big.set_generation(0, 1.0, repetition_penalty=1.1)
    assert e.value.code == 2 and big.generation(0)["min_p"] == np.float32(0.05)
    big.close()
