"""MXFP4 against int8 at batch-1 decode: Llama-2-7B at ctx 2048 (KV filled to position ctx - 2, the idempotent step
at ctx - 1, as bench.py), built once per weight type in the same process and timed in interleaved rounds
(sli_model_time_steps, sli_model_time_families). Prints one JSON line: tok/s per type and their ratio, and per
kernel family the mean device us per launch and GB/s against the algorithmic bytes (mxfp4: cols / 2 + cols / 32
bytes per row).

    python tools/mxfp4_time.py [--rounds 3] [--iters 20] [--layers 32] [--ctx 2048]

--prefill: the prompt prefill instead. One process, a 512-token prompt, three configurations timed in interleaved
rounds: the MXFP4 model after set_prefill("gemm") (pgemm_kernel<…, mxfp4>), the same model on the decode step
(set_prefill("decode"), one weight pass per prompt token) and the int8 model's GEMM prefill. A time is the host clock
around sli_model_prefill, which ends in a stream synchronise; every configuration is warmed up once first (graph
capture, code objects), the GEMM legs repeat --reps times per round so a window is a fraction of a second at least.
Prints one JSON line with the median round of each and writes it to --out (profiles/mxfp4_prefill.json).

    python tools/mxfp4_time.py --prefill [--tokens 512] [--rounds 3] [--reps 8] [--out profiles/mxfp4_prefill.json]

--batch B (2..8): the batched step instead. The MXFP4 model (opt-in, mx_batch=True) and the int8 model of --preset are
built in ONE process (same seed; KV filled to ctx - 2, the idempotent step at ctx - 1 for every sequence) and, after a
settle of replayed steps as in tools/kv8_time.py, timed in interleaved rounds. Writes --out
(profiles/mxfp4_batch_time.json): per weight type the step us and tok/s (median round, every round, min and max), the
per-family launch times (median, min, max over the rounds) and the step's bytes; then the ratio of the medians,
counted as a difference only if the gap exceeds the spread (max - min) of the int8 model's own rounds. A record, not a
gate. It is one GPU process: run it under a time limit of its own, chained with && to whatever follows:

    timeout -k 10 900 python tools/mxfp4_time.py --batch 8 --preset llama3-8b --ctx 4096 [--kv f16] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def prefill_leg(a):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b", num_hidden_layers=a.layers, max_length=a.ctx)
    n = a.tokens
    ids = [(1 + 7919 * i) % cfg.vocab_size for i in range(n)]
    mxm = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=1).init()
    i8m = LlamaModel(config=cfg, w_dtype="i8", kv_dtype="f16", seed=1).init()
    legs = {"mxfp4_gemm": (mxm, "gemm", a.reps), "mxfp4_decode": (mxm, "decode", 1), "i8_gemm": (i8m, "auto", a.reps)}
    paths = {}

    def run(name):
        m, mode, reps = legs[name]
        m.set_prefill(mode)
        paths[name] = m.prefill_path()
        t = time.perf_counter()
        for _ in range(reps):
            m.prefill(ids)  # returns after the stream synchronise
        return (time.perf_counter() - t) / reps * 1e3

    for name in legs:  # warm-up: graph capture, code objects, the decode graph
        run(name)
    ms = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name in legs:  # interleaved: the three see the same clocks and neighbours
            ms[name].append(run(name))
    assert paths == {"mxfp4_gemm": "mfma", "mxfp4_decode": "decode", "i8_gemm": "mfma"}, paths
    out = {"model": "llama2-7b", "layers": a.layers, "prompt_tokens": n, "prefilled_positions": n - 1,
           "rounds": a.rounds, "reps_gemm": a.reps, "clock": "host, around sli_model_prefill (synchronises)"}
    for name in legs:
        med = sorted(ms[name])[len(ms[name]) // 2]
        out[name] = {"ms": round(med, 2), "ms_rounds": [round(v, 2) for v in ms[name]],
                     "tok_s": round((n - 1) / (med * 1e-3), 0), "path": paths[name]}
    out["speedup_mxfp4_gemm_over_decode"] = round(out["mxfp4_decode"]["ms"] / out["mxfp4_gemm"]["ms"], 2)
    out["tok_s_ratio_mxfp4_gemm_over_i8_gemm"] = round(out["i8_gemm"]["ms"] / out["mxfp4_gemm"]["ms"], 4)
    mxm.close()
    i8m.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def settle(m, ms):
    t0 = time.perf_counter()
    while True:
        for _ in range(8):
            m.step()
        m.sync()
        if (time.perf_counter() - t0) * 1e3 >= ms:
            return


def batched_leg(a):
    import torch  # noqa: F401  (before the library, as tools/kv8_time.py explains)
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset(a.preset, num_hidden_layers=a.layers, max_length=a.ctx)
    kinds = ("mxfp4", "i8")
    models = {}
    for w in kinds:
        m = LlamaModel(config=cfg, w_dtype=w, kv_dtype=a.kv, seed=1, batch=a.batch, mx_batch=(w == "mxfp4")).init()
        m.fill_kv_synthetic(7, a.ctx - 1)
        for b in range(a.batch):
            m.set_state_seq(b, (1234 + 17 * b) % cfg.vocab_size, a.ctx - 1, advance=False)
        m.step()
        m.sync()
        assert all(m.state(b)["error"] == 0 for b in range(a.batch))
        models[w] = m
    for w in kinds:
        settle(models[w], a.settle_ms)
    step_us = {w: [] for w in kinds}
    fam = {w: [] for w in kinds}
    for _ in range(a.rounds):
        for w in kinds:  # interleaved: both models see the same clocks and neighbours
            step_us[w].append(models[w].time_steps(a.iters))
        for w in kinds:
            fam[w].append(models[w].time_families(a.iters))
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"model": a.preset, "batch": a.batch, "ctx": a.ctx, "kv_dtype": a.kv, "layers": cfg.num_hidden_layers,
           "rounds": a.rounds, "iters": a.iters, "settle_ms": a.settle_ms}
    for w in kinds:
        us = step_us[w]
        wb, kb = models[w].step_bytes()
        fams = {}
        for f in LlamaModel.FAMILIES:
            v = [r[f]["avg_us"] for r in fam[w]]
            fams[f] = {"us": round(med(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                       "bytes_per_launch": fam[w][0][f]["bytes_per_launch"]}
        out[w] = {"step_us": round(med(us), 1), "step_us_rounds": [round(v, 1) for v in us],
                  "tok_s": round(a.batch * 1e6 / med(us), 1), "tok_s_min": round(a.batch * 1e6 / max(us), 1),
                  "tok_s_max": round(a.batch * 1e6 / min(us), 1), "weight_bytes": wb, "kv_bytes": kb,
                  "exec": models[w].exec_mode(), "families_us": fams}
    i8, mx = out["i8"], out["mxfp4"]
    spread = max(i8["step_us_rounds"]) - min(i8["step_us_rounds"])
    gap = i8["step_us"] - mx["step_us"]
    out["claim"] = {"tok_s_ratio_mxfp4_over_i8": round(mx["tok_s"] / i8["tok_s"], 4),
                    "weight_bytes_ratio_mxfp4_over_i8": round(mx["weight_bytes"] / i8["weight_bytes"], 4),
                    "step_gap_us_i8_minus_mxfp4": round(gap, 1), "i8_spread_us": round(spread, 1),
                    "mxfp4_faster": bool(gap > spread), "mxfp4_slower": bool(-gap > spread)}
    for m in models.values():
        m.close()
    path = a.out or "profiles/mxfp4_batch_time.json"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1, help="2..8: the batched step (MXFP4 opt-in against int8)")
    ap.add_argument("--preset", default="llama2-7b", help="the batched step's model preset")
    ap.add_argument("--kv", default="f16", choices=("f16", "f32", "f8"), help="the batched step's cache type")
    ap.add_argument("--settle-ms", type=float, default=1000.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--prefill", action="store_true", help="time the prompt prefill instead of the decode step")
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default="", help="default: profiles/mxfp4_prefill.json, or mxfp4_batch_time.json with --batch")
    a = ap.parse_args()
    if a.rounds < 2:
        ap.error("at least two interleaved rounds")
    if a.batch > 1:
        if a.rounds < 3 or a.batch > 8 or a.prefill:
            ap.error("--batch: 2..8, at least three interleaved rounds, not with --prefill")
        return batched_leg(a)
    if a.prefill:
        a.out = a.out or "profiles/mxfp4_prefill.json"
        return prefill_leg(a)
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
