"""Bit-equality of the prompt prefill across two builds of the library: this tree's (the group table is the prefill's
only row map) against another build's (--baseline-variant NAME: libsli_NAME.so, the parent commit's built with
`python -m simplellminference_amd.build --variant NAME`). Each library runs every case once in a child process of its
own, as tools/batch_prefill_time.py does, and reports per case a SHA-256 over the bytes of every layer's K and V rows
(get_kv), the per-sequence state and the logits of the first decode step (scoring: the three result arrays too).

    python tools/pf_rowmap_ab.py --baseline-variant parent [--out profiles/pf_rowmap_ab.json]

Writes both digests per case and an `equal` flag; exits non-zero unless every case is equal.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH_LENS = (300, 5, 129, 33)
# (weights, cache, set_prefill mode or None): the batch-1 configurations
B1 = (("f16", "f16", None), ("i8", "f16", None), ("i8", "f32", None), ("mxfp4", "f16", "gemm"), ("f16", "f8", "gemm-kv8"))


def _prompt(n, vocab, seed=3):
    return [int(t) for t in np.random.default_rng(seed + n).integers(0, vocab, n)]


def _digest(models, lens, step, logits, extra=()):
    """models: the engines whose cache and state count (one model, or a group's ranks); lens[b]: sequence b's prompt."""
    h = hashlib.sha256()
    step()
    for m in models:
        for b, n in enumerate(lens):
            for layer in range(m.config.num_hidden_layers):
                for which in (0, 1):
                    h.update(np.ascontiguousarray(m.kv(layer, which, n, seq=b)).tobytes())
            h.update(json.dumps(m.state(b), sort_keys=True).encode())
    h.update(np.ascontiguousarray(logits()).tobytes())
    for x in extra:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def cases():
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    cfg = preset("tiny-gqa", max_length=320)
    for w, kv, mode in B1:
        for n in (40, 300):
            m = LlamaModel(config=cfg, w_dtype=w, kv_dtype=kv, seed=0).init()
            if mode:
                m.set_prefill(mode)
            assert m.prefill_path() == "mfma"
            m.prefill(_prompt(n, cfg.vocab_size))
            yield f"prefill {w}/{kv} n={n}", _digest([m], [n], m.step, lambda: m.logits()[0])
            m.close()
    gcfg = preset("tiny-h8", max_length=320)
    g = TPGroup(gcfg, 2, w_dtype="f16", kv_dtype="f16", seed=2).init()
    assert g.prefill_path() == "mfma"
    g.prefill(_prompt(300, gcfg.vocab_size))
    yield "tp-group prefill tiny-h8 tp=2 n=300", _digest(g.ranks, [300], g.step, g.logits)
    g.close()
    prompts = [_prompt(n, cfg.vocab_size, seed=5 + b) for b, n in enumerate(BATCH_LENS)]
    for route in ("prefill_batch", "score"):
        m = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=0, batch=len(prompts)).init()
        extra = []
        if route == "score":
            for rec in m.score(prompts):
                extra += [rec["logprobs"], rec["top"], rec["top_logprobs"]]
        else:
            m.prefill_batch(prompts)
        yield f"{route} batch={len(prompts)} lens={BATCH_LENS}", _digest([m], BATCH_LENS, m.step, lambda: m.logits()[0], extra)
        m.close()


def _child(variant):
    env = {k: v for k, v in os.environ.items() if k != "SLI_LIB_VARIANT"}
    if variant:
        env["SLI_LIB_VARIANT"] = variant
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-variant", default="parent")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pf_rowmap_ab.json"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(dict(cases())))
        return 0
    base, own = _child(a.baseline_variant), _child("")
    assert list(base) == list(own)
    out = {"baseline_variant": a.baseline_variant,
           "cases": {k: {"baseline": base[k], "this_build": own[k], "equal": base[k] == own[k]} for k in own}}
    out["all_equal"] = all(c["equal"] for c in out["cases"].values())
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for k, c in out["cases"].items():
        print(f"{'equal    ' if c['equal'] else 'DIFFERENT'} {k}")
    print(f"wrote {a.out}")
    return 0 if out["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
