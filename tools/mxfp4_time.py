"""MXFP4 against int8 at batch-1 decode: Llama-2-7B at ctx 2048 (KV filled to position ctx - 2, the idempotent step
at ctx - 1, as bench.py), built once per weight type in the same process and timed in interleaved rounds
(sli_model_time_steps, sli_model_time_families). Prints one JSON line: tok/s per type and their ratio, and per
kernel family the mean device us per launch and GB/s against the algorithmic bytes (mxfp4: cols / 2 + cols / 32
bytes per row).

    python tools/mxfp4_time.py [--rounds 3] [--iters 20] [--layers 32] [--ctx 2048]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ctx", type=int, default=2048)
    a = ap.parse_args()
    if a.rounds < 2:
        ap.error("at least two interleaved rounds")
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b", num_hidden_layers=a.layers, max_length=a.ctx)
    kinds = ("i8", "mxfp4")
    models = {}
    for w in kinds:
        m = LlamaModel(config=cfg, w_dtype=w, kv_dtype="f16", seed=1).init()
        m.fill_kv_synthetic(7, a.ctx - 1)
        m.set_state(1234, a.ctx - 1, advance=False)
        m.step()
        m.sync()
        models[w] = m
    step_us = {w: [] for w in kinds}
    fam = {w: [] for w in kinds}
    for _ in range(a.rounds):
        for w in kinds:  # interleaved: both types see the same clocks and neighbours
            step_us[w].append(models[w].time_steps(a.iters))
        for w in kinds:
            fam[w].append(models[w].time_families(a.iters))
    out = {"model": "llama2-7b", "layers": a.layers, "ctx": a.ctx, "rounds": a.rounds, "iters": a.iters}
    for w in kinds:
        us = sorted(step_us[w])[len(step_us[w]) // 2]  # median round
        wb, kb = models[w].step_bytes()
        fams = {}
        for f in LlamaModel.FAMILIES:
            t = sorted(r[f]["avg_us"] for r in fam[w])[a.rounds // 2]
            b = fam[w][0][f]["bytes_per_launch"]
            fams[f] = {"us": round(t, 2), "GBps": round(b / (t * 1e-6) / 1e9, 1), "bytes": b}
        out[w] = {"tok_s": round(1e6 / us, 1), "step_us": round(us, 1), "step_us_rounds": [round(v, 1) for v in step_us[w]],
                  "weight_bytes": wb, "kv_bytes": kb, "families": fams}
    out["tok_s_ratio_mxfp4_over_i8"] = round(out["mxfp4"]["tok_s"] / out["i8"]["tok_s"], 4)
    for m in models.values():
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
