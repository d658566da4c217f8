"""The queue scenario of tests/test_gpu_generate.py, built with the oracle alone in the manner of
tests/extend_scenarios.py: eight greedy requests for a tiny-gqa model of batch 2, so every slot is reused and a queue
forms; each request's expected output is the oracle's greedy continuation of its prompt, cut behind the first of its
stop tokens.

The weight seed is chosen here, on the CPU: greedy tokens can only be held bit-equal where the oracle's top-2 logit gap
is no near tie, so of seeds 0 .. 23 the scenario takes the one with the largest minimum gap over every compared
position (the 60 positions whose logits choose a generated token). It must exceed 2e-3, twice the 1e-3 parity bar of
the engine against the oracle, so the GPU's argmax cannot differ.

    python -m tests.gen_scenarios   # prints the best seed, its gap, seed 0's and the recorded seed's

Recorded: seed 15, minimum top-2 gap 7.3e-3 (seed 0: 2.2e-3).
"""
from __future__ import annotations

import numpy as np

from tests import extend_scenarios as S

LENS = [1, 2, 5, 17, 20, 9, 3, 12]
NEW = [12, 3, 8, 5, 10, 4, 12, 6]
SEED, MIN_GAP = 15, 2e-3
# request -> which of its own oracle-decoded tokens is its stop token (at seed 15 each occurs there first, so the
# requests end after 6, 5 and 7 tokens)
STOP_AT = {0: 5, 4: 4, 6: 6}


def config():
    from simplellminference_amd.model import preset
    return preset("tiny-gqa")


def prompts(cfg):
    return [S.prompt(n, cfg.vocab_size, seed=100 + i) for i, n in enumerate(LENS)]


def continuations(oracle, cfg, seed):
    """Per request the NEW[i] tokens the oracle decodes behind the prompt."""
    return [S.run(oracle, cfg, p, len(p) + k, seed)[0][len(p):].astype(np.int32) for p, k in zip(prompts(cfg), NEW)]


def scenario(oracle, cfg=None, seed=SEED):
    """(requests for model.generate, expected results)."""
    cfg = cfg or config()
    reqs, want = [], []
    for i, (p, k, cont) in enumerate(zip(prompts(cfg), NEW, continuations(oracle, cfg, seed))):
        r = {"prompt": p, "max_new_tokens": k}
        if i in STOP_AT:
            stop = int(cont[STOP_AT[i]])
            r["stop"] = (stop,)
            cut = int(np.flatnonzero(cont == stop)[0]) + 1  # its first occurrence ends the request
            want.append({"tokens": cont[:cut], "finish": "stop"})
        else:
            want.append({"tokens": cont, "finish": "length"})
        reqs.append(r)
    return reqs, want


def min_gap(oracle, cfg, seed):
    """The smallest top-2 logit gap over the positions whose logits choose a generated token."""
    ps = prompts(cfg)
    return S.min_gap(oracle, cfg, ps, [len(p) - 1 for p in ps], {len(p): len(p) + k - 1 for p, k in zip(ps, NEW)}, seed)


def main():
    import oracle
    oracle.build()
    cfg = config()
    gaps = [min_gap(oracle, cfg, seed) for seed in range(24)]
    best = int(np.argmax(gaps))
    print(f"compared positions {sum(NEW)}; best seed {best} (min top-2 gap {gaps[best]:.1e}); seed 0: {gaps[0]:.1e}; "
          f"recorded seed {SEED}: {gaps[SEED]:.1e}")
    _, want = scenario(oracle, cfg)
    print([(w["finish"], len(w["tokens"])) for w in want])


if __name__ == "__main__":
    main()
