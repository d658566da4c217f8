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

--prefill: the prompt prefill instead. Per weight type (Llama-2-7B shapes, fp16 and int8 weights) an f8-cache and an
f16-cache model are built in ONE process and a 512-token prompt is prefilled in interleaved rounds along three paths:
the f8-cache model under set_prefill("gemm-kv8") (the chunked MFMA prefill over an FP8 cache), the same model under
"decode" (one teacher-forced decode step per position, what it runs by default) and the f16-cache model's GEMM prefill.
Then one chunk's attention and q/k/v launches (M = 256 at position 256, the second chunk of that prompt) are timed per
launch for both cache types through the kernel-level entry points. --baseline-variant NAME times the f16-cache GEMM
prefill of another build of the library (libsli_NAME.so, e.g. the parent commit's) in a child process before and
after the rounds, and the claim becomes the ratio to that. Writes profiles/kv8_prefill.json. A record, not a gate.

    python tools/kv8_time.py --prefill [--rounds 3] [--tokens 512] [--layers 32] [--weights f16,i8] [--baseline-variant NAME]
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


def _prefill_ms(m, ids):
    t = time.perf_counter()
    m.prefill(ids)  # returns after the chunks (or the decode steps) have run: the call waits for the stream
    m.sync()
    return (time.perf_counter() - t) * 1e3


def _launch_us(fn, iters):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def prefill_launches(cfg, w, iters):
    """One chunk's q/k/v GEMM and attention launch per cache type: us per call at M = 256, p0 = 256, T = 512, through
    the C entry points on preallocated buffers, back to back on one stream (each call also launches the one-thread
    state kernel). floor_us: the same attention call on a trivial shape, i.e. what the host and the launches cost; a
    figure near it says nothing about the kernel."""
    import ctypes
    import torch
    from simplellminference_amd import _lib, ops
    hq, hkv, hd, D = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.hidden_size
    M, p0, T, N = 256, 256, 512, (hq + 2 * hkv) * hd
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    if w == "i8":
        W, rs = torch.randint(-127, 128, (N, D), device="cuda", dtype=torch.int8, generator=g), rnd(N).abs() / 4096
    else:
        W, rs = (rnd(N, D) / 64).half(), None
    hi, lo = ops.prefill_norm_split(rnd(M, D), None, 1e-5)
    sin_t, cos_t = ops.rope_cache(hd, T, 10000.0)
    q = rnd(M, hq * hd)
    ohi = torch.zeros(M, hq * hd, device="cuda", dtype=torch.float16)
    olo = torch.zeros_like(ohi)
    st = torch.zeros(48, device="cuda", dtype=torch.int32)  # SLI_PF_TABLE_BYTES
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wdt = _lib.DT_I8 if w == "i8" else _lib.DT_F16
    out = {}
    for kv in ("f16", "f8"):
        if kv == "f16":
            kc, vc, dt = rnd(hkv, T, hd).half(), rnd(hkv, T, hd).half(), _lib.DT_F16
        else:
            kc, vc, dt = ops.quant_f8(rnd(hkv, T, hd)), ops.quant_f8(rnd(hkv, T, hd)), _lib.DT_F8E4M3
        e = _lib.PgemmEpilogue(role=0, q=q.data_ptr(), kc=kc.data_ptr(), vc=vc.data_ptr(), kv_dtype=dt,
                               sin_t=sin_t.data_ptr(), cos_t=cos_t.data_ptr(), hq=hq, hkv=hkv, hd=hd, T=T)
        qkv = lambda: _lib.call("sli_prefill_gemm", P(W), wdt, P(rs), P(hi), P(lo), N, D, M, p0, M, ctypes.byref(e), P(st),
                                None, stream)
        att = lambda M_=M, p0_=p0, hq_=hq, hkv_=hkv: _lib.call("sli_prefill_attn", P(q), P(kc), P(vc), dt, P(ohi), P(olo),
                                                              M_, M_, p0_, hq_, hkv_, hd, T, P(st), stream)
        out[kv] = {"qkv_us": round(_launch_us(qkv, iters), 2), "attention_us": round(_launch_us(att, iters), 2),
                   "floor_us": round(_launch_us(lambda: att(32, 0, 1, 1), iters), 2)}
    return out


def _baseline_child(a, w, variant):
    """The f16-cache GEMM prefill of libsli_<variant>.so (variant "": this build's libsli.so), timed by a fresh child
    process of this tool: one model, prefills back to back."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k != "SLI_LIB_VARIANT"}
    if variant:
        env["SLI_LIB_VARIANT"] = variant
    cmd = [sys.executable, os.path.abspath(__file__), "--prefill-f16-only", "--weights", w, "--rounds", str(a.rounds),
           "--tokens", str(a.tokens), "--layers", str(a.layers)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"baseline child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_rounds"]


def prefill_f16_only(a):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b", num_hidden_layers=a.layers)
    ids = [(1 + 7919 * i) % cfg.vocab_size for i in range(a.tokens)]
    m = LlamaModel(config=cfg, w_dtype=a.weights, kv_dtype="f16", seed=1).init()
    assert m.prefill_path() == "mfma"
    _prefill_ms(m, ids)  # captures the chunk graphs
    ms = [_prefill_ms(m, ids) for _ in range(a.rounds)]
    m.close()
    print(json.dumps({"ms_rounds": [round(v, 3) for v in ms]}))


def run_prefill(w, a):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b", num_hidden_layers=a.layers)
    ids = [(1 + 7919 * i) % cfg.vocab_size for i in range(a.tokens)]
    med = lambda v: sorted(v)[len(v) // 2]
    base = _baseline_child(a, w, a.baseline_variant) if a.baseline_variant else []
    own = _baseline_child(a, w, "") if a.baseline_variant else []
    m8 = LlamaModel(config=cfg, w_dtype=w, kv_dtype="f8", seed=1).init()
    m16 = LlamaModel(config=cfg, w_dtype=w, kv_dtype="f16", seed=1).init()
    paths = {"f8_gemm_kv8": (m8, "gemm-kv8", "mfma"), "f8_decode": (m8, "decode", "decode"), "f16_gemm": (m16, "auto", "mfma")}
    ms = {k: [] for k in paths}
    for r in range(-1, a.rounds):  # round -1: the warm-up that captures the graphs of every path
        for k, (m, mode, path) in paths.items():  # interleaved: the paths see the same clocks and neighbours
            m.set_prefill(mode)
            assert m.prefill_path() == path, (k, m.prefill_path())
            t = _prefill_ms(m, ids)
            assert m.state()["error"] == 0
            if r >= 0:
                ms[k].append(t)
    m8.close()
    m16.close()
    if a.baseline_variant:  # again after the rounds, in the other order
        own += _baseline_child(a, w, "")
        base += _baseline_child(a, w, a.baseline_variant)
    out = {"model": "llama2-7b", "w_dtype": w, "tokens": a.tokens, "layers": a.layers,
           "paths_ms": {k: {"ms": round(med(v), 3), "ms_rounds": [round(x, 3) for x in v]} for k, v in ms.items()},
           "launches_us": prefill_launches(cfg, w, a.iters)}
    g8, dec, g16 = (med(ms[k]) for k in ("f8_gemm_kv8", "f8_decode", "f16_gemm"))
    out["claim"] = {"f8_gemm_over_f16_gemm": round(g8 / g16, 4), "f8_decode_over_f8_gemm": round(dec / g8, 2)}
    if base:
        out["baseline"] = {"variant": a.baseline_variant, "f16_gemm_ms": round(med(base), 3),
                           "ms_rounds": [round(x, 3) for x in base]}
        out["claim"]["f8_gemm_over_baseline_f16_gemm"] = round(g8 / med(base), 4)
        # the same child process with this build's library: the f16-cache path of the two builds under one condition
        # (the in-process figure above shares its rounds with two other paths and a second resident model)
        out["baseline"]["this_build_f16_gemm_ms"] = round(med(own), 3)
        out["baseline"]["this_build_ms_rounds"] = [round(x, 3) for x in own]
        out["claim"]["f16_gemm_child_over_baseline_f16_gemm"] = round(med(own) / med(base), 4)
    return out


def main_prefill(a):
    # torch before the library (as tests/conftest.py and bench.py load them): the torch wheel bundles a ROCm runtime of
    # its own under the system runtime's sonames, so whichever is loaded first serves the whole process, and torch's
    # libraries need theirs. Loaded second, torch ran on the system runtime and the process aborted in its exit
    # handlers ("double free or corruption") after the results were written.
    import torch  # noqa: F401
    out = {"rounds": a.rounds, "iters": a.iters, "prefill": {}}
    path = a.out or "profiles/kv8_prefill.json"
    for w in a.weights.split(","):
        out["prefill"][w] = run_prefill(w, a)
        print(w, json.dumps(out["prefill"][w]["claim"]), json.dumps(out["prefill"][w]["launches_us"]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefill", action="store_true", help="time the prompt prefill paths (profiles/kv8_prefill.json)")
    ap.add_argument("--prefill-f16-only", action="store_true", help=argparse.SUPPRESS)  # the baseline child
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--weights", default="f16,i8")
    ap.add_argument("--baseline-variant", default="", help="also time libsli_<NAME>.so's f16-cache GEMM prefill")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--settle-ms", type=float, default=1000.0)
    ap.add_argument("--configs", default="c4_f16,c4_i8,c1_f16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("at least three interleaved rounds")
    if a.prefill_f16_only:
        return prefill_f16_only(a)
    if a.prefill:
        return main_prefill(a)
    a.out = a.out or "profiles/kv8_time.json"
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
