"""What sampling inside the step costs: the greedy step against the sampling step, and the sampler launch alone.

One process. C1 (Llama-2-7B fp16, batch 1, ctx 2048) and C4 (llama3-8b fp16, batch 8, ctx 4096) are built in turn (KV
filled to ctx - 2, the idempotent step at ctx - 1 for every sequence, as bench.py); each times the greedy step and
four sampling settings (T only, top-k 50, top-p 0.9, top-k 50 + top-p 0.9) in three interleaved rounds of
sli_model_time_steps. Switching between greedy and sampling re-captures the step graph (untimed); every leg replays
--settle steps before its window. The logits come from the synthetic weights and are nearly flat, the worst case for
the top-p passes (every element of the row carries mass; a trained model's nucleus is a small part of the row).

Then the sampler launch alone: ops.sample back to back between HIP events over N(0, 2.5^2) logits at V 32 000 x 1 row
and V 128 256 x 8 rows, the same four settings, mean us per launch (median of the rounds).

--ab-log FILE: the output of `tools/ab_variants.sh "base parent" ...` from the same session (the greedy bench line of
this tree against a variant build of the parent commit, interleaved); its tok/s values are recorded per variant.

Writes --out (profiles/sample_time.json) and prints it as one JSON line. A record, not a gate. One GPU process: run it
under a time limit of its own, chained with && to whatever follows:

    timeout -k 10 600 python tools/sample_time.py [--rounds 3] [--iters 20] [--layers 32] [--ab-log FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = {"greedy": None, "T": (0.8, 0, 1.0), "top_k": (0.8, 50, 1.0), "top_p": (0.8, 0, 0.9),
            "top_k_top_p": (0.8, 50, 0.9)}


def med(v):
    return sorted(v)[len(v) // 2]


def summary(v, digits=1):
    return {"us": round(med(v), digits), "rounds": [round(x, digits) for x in v]}


def step_leg(a, name, preset_name, batch, ctx):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset(preset_name, num_hidden_layers=a.layers, max_length=ctx)
    m = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=1, batch=batch).init()
    m.fill_kv_synthetic(7, ctx - 1)
    for b in range(batch):
        m.set_state_seq(b, (1234 + 17 * b) % cfg.vocab_size, ctx - 1, advance=False)
    us = {s: [] for s in SETTINGS}
    sampled = {}
    for _ in range(a.rounds):
        for s, prm in SETTINGS.items():  # interleaved: every setting sees the same clocks and neighbours
            if prm is None:
                m.set_sampling(None)
            else:
                m.set_sampling(prm[0], top_k=prm[1], top_p=prm[2], seed=1)
            for _ in range(a.settle):
                m.step()
            m.sync()
            us[s].append(m.time_steps(a.iters))
            sampled[s] = [m.sampled(b) for b in range(batch)]
    assert all(m.state(b)["error"] == 0 for b in range(batch))
    out = {"model": preset_name, "batch": batch, "ctx": ctx, "layers": cfg.num_hidden_layers,
           "vocab": cfg.vocab_size, "step_us": {s: summary(v) for s, v in us.items()}, "sampled": sampled}
    g = out["step_us"]["greedy"]
    out["greedy_spread_us"] = round(max(g["rounds"]) - min(g["rounds"]), 1)
    out["sampling_minus_greedy_us"] = {s: round(out["step_us"][s]["us"] - g["us"], 1) for s in SETTINGS if s != "greedy"}
    m.close()
    print(f"{name}: {json.dumps(out['step_us'])}", file=sys.stderr, flush=True)
    return out


def launch_leg(a, V, rows):
    import torch
    from simplellminference_amd import ops
    g = torch.Generator(device="cuda").manual_seed(V)
    logits = torch.randn(rows, V, device="cuda", generator=g) * 2.5
    pos = torch.full((rows,), 2047, dtype=torch.int32, device="cuda")
    tok = torch.empty(rows, dtype=torch.int32, device="cuda")
    out = {}
    for s, prm in SETTINGS.items():
        if prm is None:
            continue
        run = lambda: ops.sample(logits, prm[0], prm[1], prm[2], 1, pos, out=tok)
        for _ in range(10):
            run()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launch_iters):
                run()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.launch_iters)
        out[s] = summary(us, 2)
    return {"vocab": V, "rows": rows, "launches_per_window": a.launch_iters, "launch_us": out}


def ab_lines(path):
    """`<variant> <tok/s> {family: us, ...}` lines of tools/ab_variants.sh, in order."""
    runs = {}
    for line in open(path):
        f = line.split()
        if len(f) >= 2 and f[0] in ("base", "parent"):
            try:
                runs.setdefault(f[0], []).append(float(f[1]))
            except ValueError:
                pass
    out = {v: {"tok_s_rounds": r, "step_us_rounds": [round(1e6 / x, 1) for x in r]} for v, r in runs.items()}
    if "base" in out and "parent" in out:
        p = out["parent"]["step_us_rounds"]
        out["parent_spread_us"] = round(max(p) - min(p), 1)
        out["base_minus_parent_us"] = round(med(out["base"]["step_us_rounds"]) - med(p), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--settle", type=int, default=40, help="untimed steps before each window")
    ap.add_argument("--launch-iters", type=int, default=200)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ab-log", default="", help="output of tools/ab_variants.sh \"base parent\" from this session")
    ap.add_argument("--out", default="profiles/sample_time.json")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three interleaved rounds")
    import torch  # noqa: F401  (before the library, as tools/kv8_time.py explains)
    out = {"rounds": a.rounds, "iters": a.iters, "settle_steps": a.settle,
           "settings": {s: (None if p is None else {"temperature": p[0], "top_k": p[1], "top_p": p[2]})
                        for s, p in SETTINGS.items()},
           "C1": step_leg(a, "C1", "llama2-7b", 1, 2048), "C4": step_leg(a, "C4", "llama3-8b", 8, 4096),
           "launch": [launch_leg(a, 32000, 1), launch_leg(a, 128256, 8)]}
    if a.ab_log:
        out["greedy_vs_parent_bench"] = ab_lines(a.ab_log)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
