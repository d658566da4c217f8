"""The scenarios of tests/test_gpu_extend.py and tests/test_gpu_kv_copy.py, built with the oracle alone: for each, the
full forced token list of every sequence (prompt, the greedy tokens decoded before the continuation, the continuation)
and the first position whose logits the test compares. The GPU tests feed the same lists to the engine piecewise.

Weight seeds are chosen here, on the CPU, in the manner of tests/test_gpu_batch_prefill.py: greedy tokens can only be
held bit-equal where the oracle's top-2 logit gap is no near tie, so each scenario takes, of seeds 0 .. 23, the one
with the largest minimum gap over every compared position of every sequence.

    python -m tests.extend_scenarios [name ...]   # prints, per scenario, the best seed, its gap and seed 0's

prints the table SEEDS below was filled from.
"""
from __future__ import annotations

import numpy as np

LENS = (1, 2, 17, 40)
# scenario -> weight seed, from the scan above. Its minimum top-2 gap over the compared positions (and seed 0's):
#   turn 3.0e-3 (1.9e-4); turn-i8 2.9e-3 (3.9e-4); rollback 1.2e-2 (3.1e-3); admit 7.3e-3 (6.4e-3); one 5.9e-3 (5.6e-4);
#   one-f32kv 5.9e-3 (4.8e-4); one-tp 1.9e-2 (3.1e-3); edge 2.2e-2 (seed 0 itself); fork 1.1e-2 (2.6e-5);
#   again 3.5e-2 (1.0e-2); again-f32kv 3.5e-2 (1.0e-2); again-tp 5.3e-2 (3.2e-2)
SEEDS = {"turn": 21, "turn-i8": 17, "rollback": 15, "admit": 15, "one": 17, "one-f32kv": 17, "one-tp": 17, "edge": 0,
         "fork": 20, "again": 10, "again-f32kv": 10, "again-tp": 21}


def ocfg(oracle, cfg):
    return oracle.Config(cfg.vocab_size, cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads,
                         cfg.head_dim, cfg.intermediate_size, cfg.num_hidden_layers, cfg.max_length,
                         cfg.rms_norm_eps, cfg.rope_theta)


def prompt(n, vocab, seed=3):  # tests/test_gpu_batch_prefill.py's _prompt
    return [int(t) for t in np.random.default_rng(seed + n).integers(0, vocab, n)]


def run(oracle, cfg, forced, steps, seed, wmode=None, kv_f16=True, kv=False):
    """The oracle's predict over a forced list: (tokens [steps], logits [steps, V], (K, V) rows or None)."""
    om = oracle.Model(ocfg(oracle, cfg), seed=seed, wmode=oracle.W_F16 if wmode is None else wmode, kv_f16=kv_f16)
    tok, log = om.predict(forced, steps)
    rows = tuple(a.copy() for a in om.kv_cache()) if kv else None
    om.close()
    return tok, log, rows


def decoded(oracle, cfg, p, k, seed, **kw):
    """Prompt p and the k tokens the oracle decodes behind it: positions 0 .. len(p) + k - 1, the last one pending."""
    return [int(t) for t in run(oracle, cfg, p, len(p) + k, seed, **kw)[0]]


def turn(oracle, cfg, seed, **kw):
    """Test 3: prompts of LENS, 6 decode steps, then 3 tokens appended to sequence 1 and 20 to sequence 2. Returns
    (forced lists, first compared position per sequence)."""
    lists = [decoded(oracle, cfg, prompt(n, cfg.vocab_size), 6, seed, **kw) for n in LENS]
    lists[1] += prompt(3, cfg.vocab_size, seed=99)
    lists[2] += prompt(20, cfg.vocab_size, seed=99)
    return lists, [n - 1 for n in LENS]


def rollback(oracle, cfg, seed, **kw):
    """Test 4: after the turn, sequence 2 goes back to position 20 and takes 9 other tokens. Compared from 16 on, the
    first position it decoded: the tokens at 17 .. 19 that the rollback keeps are greedy ones."""
    lists, _ = turn(oracle, cfg, seed, **kw)
    return [lists[2][:20] + prompt(9, cfg.vocab_size, seed=77)], [16]


ADMIT_LENS, ADMIT_N, ADMIT_BETWEEN, ADMIT_AFTER = (5, 33, 17), 300, 6, 10


def admit(oracle, cfg, seed, **kw):
    """Test 5: three running sequences (6 steps while sequence 3 is admitted, 10 after) and the 300-token prompt."""
    ps = [prompt(n, cfg.vocab_size) for n in ADMIT_LENS] + [prompt(ADMIT_N, cfg.vocab_size, seed=5)]
    return ps, [len(p) - 1 for p in ps]


def one(oracle, cfg, seed, **kw):
    """Test 7: a 20-token prompt, 3 decode steps, a 12-token turn."""
    return [decoded(oracle, cfg, prompt(20, cfg.vocab_size), 3, seed, **kw) + prompt(12, cfg.vocab_size, seed=99)], [19]


def edge(oracle, cfg, seed, **kw):
    """Test 8 (max_length 40): a 36-token prompt continued from 35 with 3 tokens; a 20-token prompt continued from 19
    up to the last position."""
    v = cfg.vocab_size
    return [prompt(36, v) + prompt(3, v, seed=99), prompt(20, v) + prompt(20, v, seed=99)], [35, 19]


def fork(oracle, cfg, seed, **kw):
    """Test 9: a 30-token prompt; its first 20 rows copied, 7 tokens appended behind token 20."""
    p = prompt(30, cfg.vocab_size)
    return [p, p[:21] + prompt(7, cfg.vocab_size, seed=99)], [29, 20]


AGAIN = ((40, 46), (9, 15))  # (prompt length, predict length) of the two calls


def again(oracle, cfg, seed, **kw):
    """A 40-token prompt predicted to 46, then on the same model a 9-token prompt predicted to 15: two independent
    oracle runs, each compared from its last prompt position on."""
    return [prompt(n, cfg.vocab_size) for n, _ in AGAIN], [n - 1 for n, _ in AGAIN]


def min_gap(oracle, cfg, lists, first, steps, seed, **kw):
    from tests.score_ref import top2_gap
    g = np.inf
    for forced, f in zip(lists, first):
        n = steps if isinstance(steps, int) else steps[len(forced)]
        _, log, _ = run(oracle, cfg, forced, n, seed, **kw)
        g = min(g, min(top2_gap(log[t]) for t in range(f, n)))
    return g


def scenarios(oracle):
    from simplellminference_amd.model import preset
    g, g320, g40, h8 = preset("tiny-gqa"), preset("tiny-gqa", max_length=320), preset("tiny-gqa", max_length=40), \
        preset("tiny-h8")
    admit_steps = {n: n + ADMIT_BETWEEN + ADMIT_AFTER for n in ADMIT_LENS}
    admit_steps[ADMIT_N] = ADMIT_N + ADMIT_AFTER
    return {
        "turn": (g, turn, 64, {}),
        "turn-i8": (g, turn, 64, dict(wmode=oracle.W_I8)),
        "rollback": (g, rollback, 64, {}),
        "admit": (g320, admit, admit_steps, {}),
        "one": (g, one, 64, {}),
        "one-f32kv": (g, one, 64, dict(kv_f16=False)),
        "one-tp": (h8, one, 64, {}),
        "edge": (g40, edge, 40, {}),
        "fork": (g, fork, 64, {}),
        "again": (g, again, dict(AGAIN), {}),
        "again-f32kv": (g, again, dict(AGAIN), dict(kv_f16=False)),
        "again-tp": (h8, again, dict(AGAIN), {}),
    }


def main():
    import sys

    import oracle
    oracle.build()
    for name, (cfg, build, steps, kw) in scenarios(oracle).items():
        if sys.argv[1:] and name not in sys.argv[1:]:
            continue
        gaps = []
        for seed in range(24):
            lists, first = build(oracle, cfg, seed, **kw)
            gaps.append(min_gap(oracle, cfg, lists, first, steps, seed, **kw))
        best = int(np.argmax(gaps))
        print(f"{name:10s} best seed {best:2d} (min top-2 gap {gaps[best]:.1e}); seed 0: {gaps[0]:.1e}; "
              f"recorded seed {SEEDS[name]}: {gaps[SEEDS[name]]:.1e}")


if __name__ == "__main__":
    main()
