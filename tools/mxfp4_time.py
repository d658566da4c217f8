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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--prefill", action="store_true", help="time the prompt prefill instead of the decode step")
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default="profiles/mxfp4_prefill.json")
    a = ap.parse_args()
    if a.rounds < 2:
        ap.error("at least two interleaved rounds")
    if a.prefill:
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
