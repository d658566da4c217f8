"""The FP8 E4M3 K/V cache against the fp16 cache at decode: per config, the f16-cache and the f8-cache model are
built in ONE process (same weights, same seed; KV filled to position ctx - 2, the idempotent step at ctx - 1, as
bench.py) and timed in interleaved rounds after a settle of replayed steps (sli_model_time_steps,
sli_model_time_families, sli_model_time_stream).

Configs: Llama-3-8B batch 8 ctx 4096 with fp16 and with int8 weights (C4), Llama-2-7B batch 1 ctx 2048 fp16 (C1).

Writes profiles/kv8_time.json: per config and cache type the step us and tok/s (median round, every round listed),
and for the attention family its us per launch (every round), its bytes per launch and its stream floor; then the
claim: the f8 attention launch against the f16 launch of the same process, counted as faster only if the gap of the
medians exceeds the spread (max - min) of the f16 launch's own rounds.

    python tools/kv8_time.py [--rounds 3] [--iters 20] [--layers 32] [--configs c4_f16,c4_i8,c1_f16] [--out ...]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"c4_f16": ("llama3-8b", "f16", 8, 4096), "c4_i8": ("llama3-8b", "i8", 8, 4096),
           "c1_f16": ("llama2-7b", "f16", 1, 2048)}


def settle(m, ms):
    t0 = time.perf_counter()
    while True:
        for _ in range(8):
            m.step()
        m.sync()
        if (time.perf_counter() - t0) * 1e3 >= ms:
            return


def run_config(name, a):
    from simplellminference_amd.model import LlamaModel, preset
    pname, w, B, ctx = CONFIGS[name]
    cfg = preset(pname, num_hidden_layers=a.layers, max_length=ctx)
    kinds = ("f16", "f8")
    models = {}
    for kv in kinds:
        m = LlamaModel(config=cfg, w_dtype=w, kv_dtype=kv, seed=1, batch=B).init()
        m.fill_kv_synthetic(7, ctx - 1)
        for b in range(B):
            m.set_state_seq(b, (1234 + 17 * b) % cfg.vocab_size, ctx - 1, advance=False)
        m.step()
        m.sync()
        assert all(m.state(b)["error"] == 0 for b in range(B))
        models[kv] = m
    for kv in kinds:
        settle(models[kv], a.settle_ms)
    step_us = {kv: [] for kv in kinds}
    fam = {kv: [] for kv in kinds}
    for _ in range(a.rounds):
        for kv in kinds:  # interleaved: both caches see the same clocks and neighbours
            step_us[kv].append(models[kv].time_steps(a.iters))
        for kv in kinds:
            fam[kv].append(models[kv].time_families(a.iters))
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"model": pname, "w_dtype": w, "batch": B, "ctx": ctx, "layers": a.layers}
    for kv in kinds:
        m = models[kv]
        us = med(step_us[kv])
        wb, kb = m.step_bytes()
        att = [r["attention"]["avg_us"] for r in fam[kv]]
        floor = m.time_stream(a.iters)["attention"]
        out[kv] = {"step_us": round(us, 1), "step_us_rounds": [round(v, 1) for v in step_us[kv]],
                   "tok_s": round(B * 1e6 / us, 1), "weight_bytes": wb, "kv_bytes": kb,
                   "exec": m.exec_mode(), "fused_qkv_attn": m.fused_qkv_attn(),
                   "attention": {"us": round(med(att), 2), "us_rounds": [round(v, 2) for v in att],
                                 "bytes_per_launch": fam[kv][0]["attention"]["bytes_per_launch"],
                                 "GBps": round(fam[kv][0]["attention"]["bytes_per_launch"] / (med(att) * 1e-6) / 1e9, 1),
                                 "stream_floor_us": round(floor, 2)},
                   "families_us": {f: round(med([r[f]["avg_us"] for r in fam[kv]]), 2) for f in LlamaModel.FAMILIES}}
    a16, a8 = out["f16"]["attention"], out["f8"]["attention"]
    spread = max(a16["us_rounds"]) - min(a16["us_rounds"])
    gap = a16["us"] - a8["us"]
    out["claim"] = {"f16_attention_us": a16["us"], "f8_attention_us": a8["us"], "gap_us": round(gap, 2),
                    "f16_spread_us": round(spread, 2), "f8_attention_faster": bool(gap > spread),
                    "tok_s_ratio_f8_over_f16": round(out["f8"]["tok_s"] / out["f16"]["tok_s"], 4)}
    for m in models.values():
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--settle-ms", type=float, default=1000.0)
    ap.add_argument("--configs", default="c4_f16,c4_i8,c1_f16")
    ap.add_argument("--out", default="profiles/kv8_time.json")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three interleaved rounds")
    out = {"rounds": a.rounds, "iters": a.iters, "settle_ms": a.settle_ms, "configs": {}}
    for name in a.configs.split(","):
        out["configs"][name] = run_config(name, a)
        print(name, json.dumps(out["configs"][name]["claim"]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # rewritten after every config: a partial run leaves what it measured
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
