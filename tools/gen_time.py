"""What per-sequence generation costs (sli_model_set_gen_seq, csrc/gen_sample.h, LlamaModel.generate). Every figure is
a record, not a promise: device-synchronised windows, every shape warmed up, interleaved rounds with their spread.

  no_regression  the greedy step and the model-level set_sampling step (T 0.8, top-k 50, top-p 0.9) at C1 (Llama-2-7B
                 fp16, batch 1, ctx 2048) and C4 (Llama-3-8B fp16, batch 8, ctx 4096) against another build's library
                 (--baseline-variant NAME: libsli_NAME.so, the parent commit's, beside libsli.so), a child process per
                 build in the order baseline, this, this, baseline. The bar is the baseline's own round-to-round spread
                 (max - min): the gap of the medians has to stay inside it ("inside_baseline_spread").
  mode           one model per configuration, the legs interleaved: the greedy step, the model-level sampling step, and
                 the per-sequence step with every row plain greedy plus a stop set (the cost of the mode itself), every
                 row sampled with the model-level settings, that plus min-p, and that plus all three penalties over
                 history windows of 64, 2048 and the full context. The history holds distinct tokens with every fourth
                 one from a set of 50 (so counts above 1 occur); the KV cache is filled to ctx - 2 and every sequence
                 steps idempotently at ctx - 1, as bench.py does.
  launch         the sampler launch alone, back to back between HIP events over N(0, 2.5^2) logits at V 32 000 x 1 row
                 and V 128 256 x 8 rows: ops.sample against ops.sample_gen with the same settings, with min-p, and with
                 the penalties over the three windows; "penalised_over_model_level" is the ratio the rocprofv3 follow-up
                 hangs on (above 2: a kernel trace of its own says which pass carries it).
  profile        where the penalised launch's time goes, asked for because it costs more than twice the model-level
                 launch: a child process under rocprofv3 --kernel-trace --stats (a run of its own) launches, at V 128 256
                 x 8 rows with the full window, the sampler with T only / top-k / top-k + top-p, each with and without
                 the penalties; the device time of every group's launches is read from the trace in dispatch order.
  queue          32 greedy requests of mixed prompt and output lengths at C4 shapes through generate(), against the same
                 requests as four fixed batches of predict_batch_prefill, each batch running to its longest member;
                 useful tokens per second for both, and what the finished() read adds to a step (steps followed by
                 finished() against steps followed by sync()).

    python tools/gen_time.py [--rounds 5] [--layers 32] [--baseline-variant NAME] [--only no_regression,mode,...]

Writes profiles/gen_time.json; a leg that --only leaves out keeps what the file already holds. A figure that was not
taken is written as "not measured".
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C1": ("llama2-7b", 1, 2048), "C4": ("llama3-8b", 8, 4096)}
SAMPLING = dict(temperature=0.8, top_k=50, top_p=0.9, seed=1)
PENALTIES = dict(repetition_penalty=1.2, presence_penalty=0.3, frequency_penalty=0.1)
med = lambda v: sorted(v)[len(v) // 2]


def _stats(v, digits=1):
    return {"us": round(med(v), digits), "rounds": [round(x, digits) for x in v],
            "spread_us": round(max(v) - min(v), digits)}


def _hist_token(i, b, vocab):
    return (1 + 7919 * (i % 50) + 11 * b) % vocab if i % 4 == 3 else (1 + 7919 * i + 104729 * b) % vocab


def _model(a, name, with_history=False):
    from simplellminference_amd.model import LlamaModel, preset
    preset_name, batch, ctx = CONFIGS[name]
    cfg = preset(preset_name, num_hidden_layers=a.layers, max_length=ctx)
    m = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=1, batch=batch).init()
    m.fill_kv_synthetic(7, ctx - 1)
    for b in range(batch):
        if with_history:  # set_state_seq records its token in the history
            for i in range(ctx - 1):
                m.set_state_seq(b, _hist_token(i, b, cfg.vocab_size), i, advance=False)
        m.set_state_seq(b, (1234 + 17 * b) % cfg.vocab_size, ctx - 1, advance=False)
    return m, cfg, batch, ctx


def _legs(m, batch, ctx):
    """name -> the call that puts the model into that leg's setting"""
    def gen(**kw):
        def f():
            for b in range(batch):
                m.set_generation(b, **kw)
        return f

    legs = {"greedy": lambda: m.set_sampling(None),
            "model_sampling": lambda: m.set_sampling(SAMPLING["temperature"], top_k=SAMPLING["top_k"],
                                                     top_p=SAMPLING["top_p"], seed=SAMPLING["seed"]),
            "gen_greedy_stop": gen(stop=(1, 2, 3), max_pos=ctx - 1),
            "gen_sampled": gen(**SAMPLING),
            "gen_min_p": gen(min_p=0.05, **SAMPLING)}
    for w in sorted({64, min(2048, ctx), ctx}):
        legs[f"gen_penalties_window_{w}"] = gen(min_p=0.05, penalty_from=ctx - w, **SAMPLING, **PENALTIES)
    return legs


def _time_legs(a, m, legs):
    us = {k: [] for k in legs}
    for r in range(-1, a.rounds):  # round -1 warms every leg up
        for k, enter in legs.items():
            enter()
            for _ in range(a.settle):
                m.step()
            m.sync()
            t = m.time_steps(a.iters)
            if r >= 0:
                us[k].append(t)
    return us


def mode(a):
    out = {}
    for name in CONFIGS:
        m, cfg, batch, ctx = _model(a, name, with_history=True)
        us = _time_legs(a, m, _legs(m, batch, ctx))
        assert all(m.state(b)["error"] == 0 and m.state(b)["pos"] == ctx - 1 for b in range(batch))
        assert m.finished().tolist() == [0] * batch
        m.close()
        o = {"model": CONFIGS[name][0], "batch": batch, "ctx": ctx, "layers": cfg.num_hidden_layers,
             "step_us": {k: _stats(v) for k, v in us.items()}}
        g, s = med(us["greedy"]), med(us["model_sampling"])
        o["minus_greedy_us"] = {k: round(med(v) - g, 1) for k, v in us.items() if k != "greedy"}
        o["minus_model_sampling_us"] = {k: round(med(v) - s, 1) for k, v in us.items() if k.startswith("gen_")}
        out[name] = o
        print(f"{name}: {json.dumps(o['step_us'])}", file=sys.stderr, flush=True)
    return out


def launch(a):
    import torch
    from simplellminference_amd import ops
    res = []
    for V, rows, ctx in ((32000, 1, 2048), (128256, 8, 4096)):
        g = torch.Generator(device="cuda").manual_seed(V)
        logits = torch.randn(rows, V, device="cuda", generator=g) * 2.5
        pos = torch.full((rows,), ctx - 1, dtype=torch.int32, device="cuda")
        hist = torch.tensor([[_hist_token(i, b, V) for i in range(ctx)] for b in range(rows)], dtype=torch.int32,
                            device="cuda")
        tok = torch.empty(rows, dtype=torch.int32, device="cuda")
        blocks = lambda **kw: [ops.gen_params(**dict(SAMPLING, **kw)) for _ in range(rows)]
        legs = {"model_level": lambda: ops.sample(logits, SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"],
                                                  SAMPLING["seed"], pos, out=tok)}
        for k, b, h in [("gen_sampled", blocks(), None), ("gen_min_p", blocks(min_p=0.05), None)] + \
                [(f"gen_penalties_window_{w}", blocks(min_p=0.05, penalty_from=ctx - w, **PENALTIES), hist)
                 for w in sorted({64, min(2048, ctx), ctx})]:
            legs[k] = (lambda b=b, h=h: ops.sample_gen(logits, b, pos, h, out=tok))
        us = {k: [] for k in legs}
        for r in range(-1, a.rounds):
            for k, run in legs.items():
                for _ in range(10):
                    run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launch_iters):
                    run()
                e1.record()
                e1.synchronize()
                if r >= 0:
                    us[k].append(e0.elapsed_time(e1) * 1e3 / a.launch_iters)
        o = {"vocab": V, "rows": rows, "ctx": ctx, "launches_per_window": a.launch_iters,
             "launch_us": {k: _stats(v, 2) for k, v in us.items()}}
        worst = max(med(v) for k, v in us.items() if k.startswith("gen_penalties"))
        o["penalised_over_model_level"] = round(worst / med(us["model_level"]), 2)
        res.append(o)
        print(json.dumps(o["launch_us"]), file=sys.stderr, flush=True)
    return res


PROFILE_GROUPS = [  # (name, penalised, sampling overrides) at V 128 256 x 8 rows, the full 4096-token window
    ("model_level_top_k_top_p", None, {}),
    ("gen_T_only", False, dict(top_k=0, top_p=1.0)),
    ("gen_top_k", False, dict(top_p=1.0)),
    ("gen_top_k_top_p", False, {}),
    ("gen_penalised_T_only", True, dict(top_k=0, top_p=1.0)),
    ("gen_penalised_top_k", True, dict(top_p=1.0)),
    ("gen_penalised_top_k_top_p", True, {}),
]
PROFILE_WARM, PROFILE_RUNS = 3, 10


def profile_child(a):
    """The launches of PROFILE_GROUPS in order, PROFILE_WARM + PROFILE_RUNS each: run under rocprofv3 --kernel-trace."""
    import torch
    from simplellminference_amd import ops
    V, rows, ctx = 128256, 8, 4096
    g = torch.Generator(device="cuda").manual_seed(V)
    logits = torch.randn(rows, V, device="cuda", generator=g) * 2.5
    pos = torch.full((rows,), ctx - 1, dtype=torch.int32, device="cuda")
    hist = torch.tensor([[_hist_token(i, b, V) for i in range(ctx)] for b in range(rows)], dtype=torch.int32,
                        device="cuda")
    tok = torch.empty(rows, dtype=torch.int32, device="cuda")
    for _, pen, over in PROFILE_GROUPS:
        s = dict(SAMPLING, **over)
        for _ in range(PROFILE_WARM + PROFILE_RUNS):
            if pen is None:
                ops.sample(logits, s["temperature"], s["top_k"], s["top_p"], s["seed"], pos, out=tok)
            else:
                ops.sample_gen(logits, [ops.gen_params(**s, **(PENALTIES if pen else {}))] * rows, pos,
                               hist if pen else None, out=tok)
        torch.cuda.synchronize()


def profile(a):
    """rocprofv3 --kernel-trace --stats over profile_child: the device time of each group's launches, from the trace's
    dispatches in order (the sampler kernels only)."""
    import csv
    import glob
    import tempfile
    d = tempfile.mkdtemp(prefix="gen_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
           os.path.abspath(__file__), "--profile-child"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"rocprofv3 failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for rec in csv.DictReader(f):
                if "sample_kernel" in rec["Kernel_Name"] or "sample_gen_kernel" in rec["Kernel_Name"]:
                    rows.append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]), rec["Kernel_Name"]))
    rows.sort()
    per = PROFILE_WARM + PROFILE_RUNS
    if len(rows) != per * len(PROFILE_GROUPS):
        raise RuntimeError(f"{len(rows)} sampler dispatches in the trace, expected {per * len(PROFILE_GROUPS)}")
    out = {"tool": "rocprofv3 --kernel-trace --stats", "vocab": 128256, "rows": 8, "window": 4096,
           "launches_per_group": PROFILE_RUNS, "kernel_us": {}}
    for i, (name, _, _) in enumerate(PROFILE_GROUPS):
        us = [(e - s) / 1e3 for s, e, _ in rows[i * per + PROFILE_WARM:(i + 1) * per]]
        out["kernel_us"][name] = _stats(us, 2)
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def queue(a):
    import numpy as np
    m, cfg, batch, ctx = _model(a, "C4")
    rng = np.random.default_rng(5)
    reqs = [{"prompt": [int(t) for t in rng.integers(0, cfg.vocab_size, int(rng.choice([16, 48, 130, 400])))],
             "max_new_tokens": int(rng.choice([8, 16, 40, 64]))} for _ in range(32)]
    useful = sum(r["max_new_tokens"] for r in reqs)

    def through_generate():
        got = m.generate(reqs)
        assert all(len(g["tokens"]) == r["max_new_tokens"] for g, r in zip(got, reqs))

    def fixed_batches():
        for i in range(0, len(reqs), batch):
            part = reqs[i:i + batch]
            m.predict_batch_prefill([r["prompt"] for r in part],
                                    max(len(r["prompt"]) + r["max_new_tokens"] for r in part))

    ms = {"generate": [], "fixed_batches": []}
    for r in range(-1, a.rounds):
        for k, fn in (("generate", through_generate), ("fixed_batches", fixed_batches)):
            if k == "fixed_batches":
                m.set_sampling(None)
            m.sync()
            t0 = time.perf_counter()
            fn()
            m.sync()
            if r >= 0:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    # what the finished() read adds to a step: the same idempotent steps, each followed by the read or by a plain sync
    for b in range(batch):
        m.set_generation(b, stop=(1,))
        m.set_state_seq(b, 5, ctx - 1, advance=False)
    per = {"step_then_sync": [], "step_then_finished": []}
    for r in range(-1, a.rounds):
        for k, after in (("step_then_sync", m.sync), ("step_then_finished", m.finished)):
            m.sync()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                m.step()
                after()
            if r >= 0:
                per[k].append((time.perf_counter() - t0) * 1e6 / a.iters)
    m.close()
    out = {"model": "llama3-8b", "layers": cfg.num_hidden_layers, "batch": batch, "requests": len(reqs),
           "generated_tokens": useful,
           **{k: {"ms": round(med(v), 2), "ms_rounds": [round(x, 2) for x in v], "spread_ms": round(max(v) - min(v), 2),
                  "tokens_per_s": round(useful / med(v) * 1e3, 1)} for k, v in ms.items()},
           "finished_read": {k: _stats(v) for k, v in per.items()}}
    out["finished_read"]["added_us_per_step"] = round(med(per["step_then_finished"]) - med(per["step_then_sync"]), 1)
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def ab_child(a):
    """The greedy and the model-level sampling step at C1 and C4 of whichever library SLI_LIB_VARIANT names."""
    out = {}
    for name in CONFIGS:
        m, cfg, batch, ctx = _model(a, name)
        legs = {k: v for k, v in _legs(m, batch, ctx).items() if k in ("greedy", "model_sampling")}
        us = _time_legs(a, m, legs)
        m.close()
        out.update({f"{name}_{k}": v for k, v in us.items()})
    print(json.dumps(out))


def _child(a, variant):
    env = {k: v for k, v in os.environ.items() if k != "SLI_LIB_VARIANT"}
    if variant:
        env["SLI_LIB_VARIANT"] = variant
    cmd = [sys.executable, os.path.abspath(__file__), "--ab-child", "--rounds", str(a.rounds), "--layers", str(a.layers),
           "--iters", str(a.iters), "--settle", str(a.settle)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def no_regression(a):
    runs = {"base": [_child(a, a.baseline_variant)], "own": [_child(a, "")]}
    runs["own"].append(_child(a, ""))
    runs["base"].append(_child(a, a.baseline_variant))
    out = {"baseline_variant": a.baseline_variant, "layers": a.layers}
    for key in runs["base"][0]:
        base = [x for r in runs["base"] for x in r[key]]
        own = [x for r in runs["own"] for x in r[key]]
        gap, spread = med(own) - med(base), max(base) - min(base)
        out[key] = {"baseline_us": round(med(base), 1), "baseline_us_rounds": [round(x, 1) for x in base],
                    "baseline_spread_us": round(spread, 1), "this_build_us": round(med(own), 1),
                    "this_build_us_rounds": [round(x, 1) for x in own], "gap_us": round(gap, 1),
                    "inside_baseline_spread": bool(abs(gap) <= spread)}
        print(f"{key}: this build {med(own):.1f} us, {a.baseline_variant} {med(base):.1f} us (its spread {spread:.1f} us)",
              file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--settle", type=int, default=20, help="untimed steps before each window")
    ap.add_argument("--launch-iters", type=int, default=200)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--baseline-variant", default="")
    ap.add_argument("--only", default="no_regression,mode,launch,profile,queue")
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--profile-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_time.json"))
    a = ap.parse_args()
    import torch
    if a.ab_child:
        return ab_child(a)
    if a.profile_child:
        return profile_child(a)
    if a.rounds < 5:
        ap.error("at least five interleaved rounds")
    if not torch.cuda.is_available():
        sys.exit("gen_time.py needs the GPU: a timing taken anywhere else says nothing")
    only = a.only.split(",")
    out = {}
    if os.path.exists(a.out):  # a leg that is not asked for keeps what an earlier call measured
        with open(a.out) as f:
            out = json.load(f)
    out.update({"rounds": a.rounds, "iters": a.iters, "settle_steps": a.settle, "sampling": SAMPLING,
                "penalties": PENALTIES})
    for k, fn in (("no_regression", no_regression), ("mode", mode), ("launch", launch), ("profile", profile),
                  ("queue", queue)):
        if k not in only:
            out.setdefault(k, "not measured")
        elif k == "no_regression" and not a.baseline_variant:
            out[k] = "not measured: no --baseline-variant"
        else:
            out[k] = fn(a)
        with open(a.out, "w") as f:  # after every leg: a later leg's failure keeps the earlier figures
            json.dump(out, f, indent=1)
            f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
