"""model.generate(requests), the queue through the batch, held to the oracle (tests/gen_scenarios.py): eight greedy
requests through a tiny-gqa model of batch 2 give the oracle's greedy continuations, cut behind the first stop token,
in request order, and again on a second call; sampled and penalised requests keep the bookkeeping and repeat bit for
bit."""
import numpy as np
import pytest

from tests import gen_scenarios as GS

pytestmark = pytest.mark.gpu


def _model(seed, batch=2):
    from simplellminference_amd.model import LlamaModel
    return LlamaModel(config=GS.config(), w_dtype="f16", kv_dtype="f16", seed=seed, batch=batch).init()


def test_the_scenario_is_no_near_tie(oracle):
    assert GS.min_gap(oracle, GS.config(), GS.SEED) > GS.MIN_GAP


def test_greedy_queue_equals_the_oracle(gpu, oracle):
    reqs, want = GS.scenario(oracle)
    assert len(reqs) >= 8 and sum(w["finish"] == "stop" for w in want) >= 2
    assert any(len(w["tokens"]) < r["max_new_tokens"] for w, r in zip(want, reqs))  # a stop ends a request early
    m = _model(GS.SEED)
    for call in range(2):  # the second call finds the model in per-sequence mode, its slots parked
        got = m.generate(reqs)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g["tokens"].dtype == np.int32 and g["tokens"].tolist() == w["tokens"].tolist(), (call, i)
            assert g["finish"] == w["finish"], (call, i)
        # left in per-sequence mode with every block cleared
        for b in range(m.batch):
            d = m.generation(b)
            assert d["temperature"] == 0.0 and d["stop"] == () and d["max_pos"] == 0 and d["repetition_penalty"] == 1.0
    m.close()


def test_requests_that_cannot_fit_raise_before_anything_runs(gpu):
    m = _model(GS.SEED)
    T = GS.config().max_length
    before = m.graph_captures()
    with pytest.raises(ValueError):
        m.generate([{"prompt": [1, 2, 3], "max_new_tokens": 4}, {"prompt": [1] * 10, "max_new_tokens": T - 9}])
    assert m.graph_captures() == before and m.state(0)["pos"] == 0
    for bad in ({"temprature": 0.5}, {"max_pos": 9}, {"stop": tuple(range(9))}):  # a misspelt or surplus keyword too
        with pytest.raises(ValueError):
            m.generate([{"prompt": [1, 2, 3], "max_new_tokens": 4}, {"prompt": [4, 5], "max_new_tokens": 2, **bad}])
        assert m.graph_captures() == before and m.state(0)["pos"] == 0 and m.generation(0)["max_pos"] == 0
    got = m.generate([{"prompt": [1] * 10, "max_new_tokens": T - 10}])  # the last position is reached
    assert got[0]["finish"] == "length" and len(got[0]["tokens"]) == T - 10
    m.close()


def test_sampled_and_penalised_queue_keeps_the_books(gpu):
    cfg = GS.config()
    rng = np.random.default_rng(4)
    reqs = []
    for i in range(10):
        n = int(rng.choice([1, 2, 7, 17, 23]))
        r = {"prompt": [int(t) for t in rng.integers(0, cfg.vocab_size, n)], "max_new_tokens": int(rng.integers(3, 13)),
             "temperature": 0.0 if i in (0, 2, 4) else float(rng.choice([0.8, 1.5])), "top_k": int(rng.choice([0, 20])),
             "top_p": float(rng.choice([1.0, 0.9])), "min_p": float(rng.choice([0.0, 0.02])),
             "repetition_penalty": float(rng.choice([1.0, 1.3])), "frequency_penalty": float(rng.choice([0.0, 0.5])),
             "presence_penalty": float(rng.choice([0.0, 0.4])), "penalty_from": int(rng.choice([0, n])),
             "stop": tuple(int(t) for t in rng.integers(0, cfg.vocab_size, 8)) if i % 2 else ()}
        reqs.append(r)
    # three requests get a stop token from their own first run, so they end early: they are the greedy (penalised) ones,
    # whose tokens do not depend on the slot they land in (a draw is seeded by its slot, and the queue's order of
    # admission changes once requests end early)
    m = _model(7, batch=3)
    first = m.generate(reqs)
    for i in (0, 2, 4):
        k = len(first[i]["tokens"]) // 2
        reqs[i]["stop"] = (int(first[i]["tokens"][k]),)
    runs = [m.generate(reqs) for _ in range(2)]
    m.close()
    stops = 0
    for i, (r, g) in enumerate(zip(reqs, runs[0])):
        toks, stop = g["tokens"].tolist(), set(r["stop"])
        if g["finish"] == "stop":
            stops += 1
            assert toks and toks[-1] in stop and not stop & set(toks[:-1]), i
            assert len(toks) <= r["max_new_tokens"], i
        else:
            assert g["finish"] == "length" and len(toks) == r["max_new_tokens"] and not stop & set(toks), i
        assert all(0 <= t < cfg.vocab_size for t in toks), i
    assert stops >= 3
    for a, b in zip(*runs):
        assert np.array_equal(a["tokens"], b["tokens"]) and a["finish"] == b["finish"]
