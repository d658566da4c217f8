"""The condition tests/test_gpu_kv8_prefill.py's model runs rest on, without a GPU: the body of
test_kv8_ref_cpu.py::test_reference_alone_fp32_against_float64 over the token sequences of those runs.

The GEMM prefill of an FP8-cache model quantises each chunk row from the q/k/v GEMM's fp32 sums, which are not the
decode step's sums, so the GPU test walks the model's codes with the float64 FP8 reference and adopts a code that
differs by one step within a slack. That is a fair comparison only if two correct implementations in different
arithmetic (here: the restatement in fp32 numpy against the one in float64) differ that way rarely, and with logits
inside the bar, on these very sequences: the long one has 312 positions, nine times the existing runs'.

Measured (flips / compared elements, slack, fp32 against float64 logits):
    tiny-gqa f16 11, n 56          0 /  28,672   6.6e-6   4.2e-7
    tiny i8 4, n 48                1 /  49,152   5.9e-6   3.9e-7
    tiny-gqa mxfp4 1, n 56         0 /  28,672   6.1e-6   3.3e-7
    small-h128-gqa i8 3, n 312     9 / 638,976   1.2e-5   1.6e-6
The cap (FLIP_CAP / 4 = 0.25 % of the compared elements) leaves two orders of magnitude of room.
"""
import numpy as np
import pytest

from tests import kv8_ref as K

PROMPT = [1, 17, 42, 99]
# (preset, weights, seed, prefilled prompt length k, positions n): the model runs of tests/test_gpu_kv8_prefill.py
PREFILL_RUNS = [("tiny-gqa", "f16", 11, 41, 56), ("tiny", "i8", 4, 34, 48), ("tiny-gqa", "mxfp4", 1, 41, 56),
                ("small-h128-gqa", "i8", 3, 300, 312)]


def run_tokens(cfg, n):
    return K.pad_prompt(PROMPT, n, cfg.vocab_size, 0)


@pytest.mark.parametrize("name,w_dtype,seed,k,n", PREFILL_RUNS)
def test_reference_alone_fp32_against_float64_prefill_runs(oracle, name, w_dtype, seed, k, n):
    from simplellminference_amd.model import preset
    cfg = preset(name)
    assert 1 < k < n <= cfg.max_length
    oc, W = K.weights(oracle, cfg, seed, w_dtype)
    toks = run_tokens(cfg, n)
    rows64, _ = K.unrounded_rows(oc, W, toks)
    rows32, _ = K.unrounded_rows(oc, W, toks, dtype=np.float32)
    slack = K.slack_from(rows64, lambda l, p, which: rows32[p][l][which])
    m32 = K.Model8(oc, W, dtype=np.float32)
    codes, logits32 = {}, []

    def adopt(l, p, which, unrounded, own):
        codes[(l, p, which)] = own
        return own
    for p, t in enumerate(toks):
        logits32.append(m32.forward(int(t), p, adopt=adopt))
    logits64, w = K.walk_run(oc, W, toks, lambda l, p, which: codes[(l, p, which)], slack)
    K.check_flips(w, f"{name} {w_dtype} n {n}", cap=K.FLIP_CAP / 4)
    K.check_logits(np.array(logits32), logits64, f"{name} {w_dtype} n {n}")
