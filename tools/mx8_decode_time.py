"""The batched MXFP4 decode step under set_decode("auto") against set_decode("mx8") (csrc/bgemm_mx8.h), beside the int8
model of tools/mxfp4_time.py --batch: one MXFP4 model (mx_batch=True) and one int8 model of --preset in ONE process (same
seed; KV filled to ctx - 2, the idempotent step at ctx - 1 for every sequence). Every round switches the MXFP4 model
auto -> mx8 (each switch re-lays the weight images and re-captures the step; one untimed step and a settle of replayed
steps follow it), and times, interleaved, the replayed step graph (sli_model_time_steps) and the five projection
launches among the kernel families (sli_model_time_families) of the three legs. Writes --out
(profiles/mx8_decode_time.json): per leg the step us and tok/s (median round, every round), the per-family launch
times (median, min, max over the rounds), then the ratios of the medians; a gap counts as a difference only if it
exceeds the spread (max - min) of the "auto" leg's own rounds. A record, not a gate. One GPU process: run it under a
time limit of its own. --auto-only times just the MXFP4 model's default step and calls nothing of the mode, so it also
runs on the parent commit's library built as a variant (SLI_LIB_VARIANT=parent): alternate the two in one session for
the A/B of the "auto" step (profiles/mx8_decode_auto_ab.json).

    timeout -k 10 900 python tools/mx8_decode_time.py --batch 8 --preset llama3-8b --ctx 4096 [--kv f16] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def settle(m, ms):
    t0 = time.perf_counter()
    while True:
        for _ in range(8):
            m.step()
        m.sync()
        if (time.perf_counter() - t0) * 1e3 >= ms:
            return


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--preset", default="llama3-8b")
    ap.add_argument("--kv", default="f16", choices=("f16", "f32", "f8"))
    ap.add_argument("--settle-ms", type=float, default=500.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ctx", type=int, default=4096)
    ap.add_argument("--out", default="profiles/mx8_decode_time.json")
    ap.add_argument("--auto-only", action="store_true",
                    help="only the MXFP4 model's default step, no set_decode call: also runs on a library without the mode "
                         "(SLI_LIB_VARIANT), for the A/B of the 'auto' step against the parent commit's library")
    a = ap.parse_args()
    if a.rounds < 3 or not 2 <= a.batch <= 8:
        ap.error("--batch 2..8, at least three interleaved rounds")
    import torch  # noqa: F401  (before the library, as tools/kv8_time.py explains)
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset(a.preset, num_hidden_layers=a.layers, max_length=a.ctx)
    models = {}
    for w in ("mxfp4",) if a.auto_only else ("mxfp4", "i8"):
        m = LlamaModel(config=cfg, w_dtype=w, kv_dtype=a.kv, seed=1, batch=a.batch, mx_batch=(w == "mxfp4")).init()
        m.fill_kv_synthetic(7, a.ctx - 1)
        for b in range(a.batch):
            m.set_state_seq(b, (1234 + 17 * b) % cfg.vocab_size, a.ctx - 1, advance=False)
        m.step()
        m.sync()
        assert all(m.state(b)["error"] == 0 for b in range(a.batch))
        models[w] = m
    if a.auto_only:
        m = models["mxfp4"]
        settle(m, a.settle_ms)
        us = [m.time_steps(a.iters) for _ in range(a.rounds)]
        m.close()
        out = {"lib_variant": os.environ.get("SLI_LIB_VARIANT", ""), "model": a.preset, "batch": a.batch, "ctx": a.ctx,
               "step_us": round(sorted(us)[len(us) // 2], 1), "step_us_rounds": [round(v, 1) for v in us]}
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")
        print(json.dumps(out))
        return
    settle(models["i8"], a.settle_ms)
    legs = ("auto", "mx8", "i8")
    step_us = {k: [] for k in legs}
    fam = {k: [] for k in legs}

    def leg(k):
        m = models["i8" if k == "i8" else "mxfp4"]
        if k != "i8":
            m.set_decode(k)
            m.step()  # re-lays the images, re-captures
            m.sync()
            assert m.decode_path() == k and all(m.state(b)["error"] == 0 for b in range(a.batch))
            settle(m, a.settle_ms)
        step_us[k].append(m.time_steps(a.iters))
        fam[k].append(m.time_families(a.iters))

    for _ in range(a.rounds):
        for k in legs:
            leg(k)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"model": a.preset, "batch": a.batch, "ctx": a.ctx, "kv_dtype": a.kv, "layers": cfg.num_hidden_layers,
           "rounds": a.rounds, "iters": a.iters, "settle_ms": a.settle_ms,
           "command": "python tools/mx8_decode_time.py " + " ".join(sys.argv[1:])}
    for k in legs:
        us = step_us[k]
        fams = {}
        for f in LlamaModel.FAMILIES:
            v = [r[f]["avg_us"] for r in fam[k]]
            fams[f] = {"us": round(med(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        out[k] = {"step_us": round(med(us), 1), "step_us_rounds": [round(v, 1) for v in us],
                  "tok_s": round(a.batch * 1e6 / med(us), 1), "families_us": fams}
    au, m8, i8 = out["auto"], out["mx8"], out["i8"]
    spread = max(au["step_us_rounds"]) - min(au["step_us_rounds"])
    gap = au["step_us"] - m8["step_us"]
    out["claim"] = {"tok_s_ratio_mx8_over_auto": round(m8["tok_s"] / au["tok_s"], 4),
                    "tok_s_ratio_mx8_over_i8": round(m8["tok_s"] / i8["tok_s"], 4),
                    "tok_s_ratio_auto_over_i8": round(au["tok_s"] / i8["tok_s"], 4),
                    "step_gap_us_auto_minus_mx8": round(gap, 1), "auto_spread_us": round(spread, 1),
                    "mx8_faster": bool(gap > spread), "mx8_slower": bool(-gap > spread),
                    "family_ratio_mx8_over_auto": {f: round(m8["families_us"][f]["us"] / au["families_us"][f]["us"], 3)
                                                   for f in LlamaModel.FAMILIES if au["families_us"][f]["us"] > 0}}
    for m in models.values():
        m.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
