"""What each weight and cache format costs in model quality, as one number per format: the same prompts scored
(LlamaModel.score, sli_model_score_seqs) by fp16, int8, MXFP4 and fp16 + FP8-cache models built from the same fp32
weights (the same synthetic seed, or --flat PATH: a real flat fp32 weight file in the reference's layout with --preset
naming its shape). Per format: mean NLL and perplexity, and against the fp16 model the mean and max |d logprob| and the
top-1 agreement (the share of scored positions whose first-max token equals fp16's).

ON SYNTHETIC WEIGHTS THE LOGITS ARE NEAR UNIFORM (mean NLL close to ln V): the table then demonstrates the pipeline, it
does not judge the formats' quality. The JSON carries that note ("synthetic": true) with the numbers.

    python tools/quant_quality.py [--layers 2] [--batch 4] [--tokens 256] [--flat PATH --preset llama2-7b] [--out ...]

Writes profiles/quant_quality.json.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMATS = (("fp16", "f16", "f16"), ("int8", "i8", "f16"), ("mxfp4", "mxfp4", "f16"), ("fp16+fp8kv", "f16", "f8"))
NOTE = ("synthetic weights: the logits are near uniform (mean NLL ~ ln V), so this table demonstrates the pipeline; "
        "it does not judge the formats' quality")


def _ids(n, b, vocab):
    return [(1 + 7919 * i + 104729 * b) % vocab for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="llama2-7b")
    ap.add_argument("--layers", type=int, default=2, help="layers of the synthetic model (ignored with --flat)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--flat", default="", help="a flat fp32 weight file (the reference's layout) of --preset's shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_quality.json"))
    a = ap.parse_args()
    import numpy as np
    from simplellminference_amd.model import LlamaModel, preset
    over = dict(max_length=a.ctx) if a.flat else dict(max_length=a.ctx, num_hidden_layers=a.layers)
    cfg = preset(a.preset, **over)
    prompts = [_ids(a.tokens, b, cfg.vocab_size) for b in range(a.batch)]
    res = {}
    for name, w, kv in FORMATS:
        m = LlamaModel(config=cfg, model_path=a.flat, w_dtype=w, kv_dtype=kv, seed=None if a.flat else a.seed,
                       batch=a.batch, mx_batch=w == "mxfp4" and a.batch > 1).init()
        if not m.score_ok():
            raise RuntimeError(f"{name}: this model cannot score")
        recs = m.score(prompts)
        m.close()
        res[name] = (np.concatenate([r["logprobs"] for r in recs]).astype(np.float64),
                     np.concatenate([r["top"] for r in recs]))
    base_lp, base_top = res["fp16"]
    rows = []
    for name, _, _ in FORMATS:
        lp, top = res[name]
        d = np.abs(lp - base_lp)
        rows.append({"format": name, "mean_nll": float(-lp.mean()), "perplexity": float(math.exp(-lp.mean())),
                     "mean_abs_dlogprob_vs_fp16": float(d.mean()), "max_abs_dlogprob_vs_fp16": float(d.max()),
                     "top1_agreement_vs_fp16": float((top == base_top).mean())})
    out = {"model": a.preset, "layers": cfg.num_hidden_layers, "batch": a.batch, "tokens": a.tokens,
           "scored_positions": int(base_lp.size), "ln_vocab": math.log(cfg.vocab_size),
           "weights": a.flat or f"synthetic seed {a.seed}", "synthetic": not a.flat, "formats": rows}
    if not a.flat:
        out["note"] = NOTE
        print("NOTE: " + NOTE)
    print(f"{'format':<12} {'mean NLL':>10} {'mean|dlp|':>10} {'max|dlp|':>10} {'top-1 agree':>12}   (ln V = {out['ln_vocab']:.4f})")
    for r in rows:
        print(f"{r['format']:<12} {r['mean_nll']:>10.5f} {r['mean_abs_dlogprob_vs_fp16']:>10.2e} "
              f"{r['max_abs_dlogprob_vs_fp16']:>10.2e} {r['top1_agreement_vs_fp16']:>12.4f}")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
