"""Prompt prefill of an MXFP4 Llama-2-7B under set_prefill("gemm") and set_prefill("gemm-mx8"), one model, one process,
rounds interleaved after warm-up runs that settle the clocks (the manner of tools/mxfp4_time.py --prefill), and the
per-launch times at M = 256 of the four GEMM roles of the block-scaled MFMA body and of the two quantisers.

    python tools/mx8_time.py [--layers 32] [--tokens 512] [--rounds 5] [--reps 4] [--out profiles/mx8_prefill.json]

--parent-variant NAME: also the unchanged "gemm" mode under this library and under libsli_NAME.so, the parent commit's
build beside it (loaded through SLI_LIB_VARIANT), a fresh process per round, the two interleaved.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _launch_us(torch, fn, n=20, reps=10):
    """Device time per launch: n calls captured in one graph (no host work between them), the graph replayed."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1e3 / (n * reps), 2)


def launches(torch, cfg, M=256):
    """One launch each at the 7B shapes, weights and activations random codes (timing only). The operands of one launch
    stay resident between replays; tools/pgemm_mx8_lab times the GEMMs with the weights streamed from HBM."""
    from simplellminference_amd import ops
    D, I, hq, hkv, hd = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    u8 = lambda *s: torch.randint(0, 120, s, device="cuda", dtype=torch.uint8)
    sc = lambda *s: torch.randint(120, 130, s, device="cuda", dtype=torch.uint8)
    W = lambda n, k: (u8(n, k // 2), sc(n, k // 32))
    A = lambda k: (u8(M, k), sc(M, k // 32))
    T = M + 16
    sin_t, cos_t = ops.rope_cache(hd, T, 10000.0)
    q, y = torch.empty(M, hq * hd, device="cuda"), torch.zeros(M, D, device="cuda")
    kc = torch.empty(hkv, T, hd, device="cuda", dtype=torch.float16)
    vc, ahi = torch.empty_like(kc), torch.empty(M, I, device="cuda", dtype=torch.float16)
    alo, x = torch.empty_like(ahi), torch.randn(M, D, device="cuda")
    wn = torch.ones(D, device="cuda")
    qkv, gu, wo, down, lm = W((hq + 2 * hkv) * hd, D), W(2 * I, D), W(D, hq * hd), W(D, I), W(cfg.vocab_size, D)
    aD, aQ, aI = A(D), A(hq * hd), A(I)
    logits = torch.empty(M, cfg.vocab_size, device="cuda")
    return {
        "qkv": _launch_us(torch, lambda: ops.prefill_gemm_qkv_mx8(*qkv, *aD, q, kc, vc, sin_t, cos_t, hq, hkv, hd, 0, M)),
        "gate_up": _launch_us(torch, lambda: ops.prefill_gemm_gate_up_mx8(*gu, *aD, ahi, alo)),
        "wo": _launch_us(torch, lambda: ops.prefill_gemm_resid_mx8(*wo, *aQ, y, resid=y)),
        "down": _launch_us(torch, lambda: ops.prefill_gemm_resid_mx8(*down, *aI, y, resid=y)),
        "logits": _launch_us(torch, lambda: ops.prefill_gemm_logits_mx8(*lm, *aD, logits)),
        "norm_quant": _launch_us(torch, lambda: ops.prefill_norm_quant_mx8(x, wn, 1e-5)),
        "pair_quant_inter": _launch_us(torch, lambda: ops.prefill_quant_mx8(ahi, alo)),
    }


def gemm_ms(a):
    """Median ms of one round of `reps` prefills under "gemm" after two warm-up rounds (a child process's whole job)."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b", num_hidden_layers=a.layers, max_length=a.tokens + 16)
    m = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=1).init()
    m.set_prefill("gemm")
    prompt = [(1 + 7919 * i) % cfg.vocab_size for i in range(a.tokens)]
    out = []
    for _ in range(3):
        m.reset()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            m.prefill(prompt)
        out.append((time.perf_counter() - t0) / a.reps * 1e3)
    m.close()
    return out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx8_prefill.json"))
    ap.add_argument("--parent-variant", default="", help="libsli_<name>.so built from the parent commit: also time "
                    '"gemm" under this library and that one, a fresh process each, rounds interleaved')
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps({"ms": gemm_ms(a)}))
        return
    import torch
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b", num_hidden_layers=a.layers, max_length=a.tokens + 16)
    m = LlamaModel(config=cfg, w_dtype="mxfp4", kv_dtype="f16", seed=1).init()
    prompt = [(1 + 7919 * i) % cfg.vocab_size for i in range(a.tokens)]
    modes = ("gemm", "gemm-mx8")

    def once(mode):
        m.set_prefill(mode)
        m.reset()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            m.prefill(prompt)  # returns after the stream has been waited for
        return (time.perf_counter() - t0) / a.reps * 1e3

    for mode in modes * 2:  # graphs captured, clocks settled
        once(mode)
    ms = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            ms[mode].append(once(mode))
    m.close()
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"model": "llama2-7b", "layers": a.layers, "tokens": a.tokens, "rounds": a.rounds, "reps": a.reps}
    for mode in modes:
        out[mode] = {"ms": round(med(ms[mode]), 3), "ms_rounds": [round(v, 3) for v in ms[mode]],
                     "tok_s": round((a.tokens - 1) / med(ms[mode]) * 1e3, 1)}
    out["time_ratio_mx8_over_gemm"] = round(out["gemm-mx8"]["ms"] / out["gemm"]["ms"], 4)
    out["gemm_spread_ms"] = round(max(ms["gemm"]) - min(ms["gemm"]), 3)
    out["launch_us_M256"] = launches(torch, cfg)
    if a.parent_variant:
        import subprocess
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--layers", str(a.layers), "--tokens", str(a.tokens),
               "--reps", str(a.reps)]
        libs = {"this": [], "parent": []}
        for _ in range(a.rounds):
            for name in libs:
                env = dict(os.environ)
                if name == "parent":
                    env["SLI_LIB_VARIANT"] = a.parent_variant
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True)
                libs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms"])
        out["gemm_vs_parent"] = {k: {"ms": round(med(v), 3), "ms_rounds": [round(x, 3) for x in v]} for k, v in libs.items()}
        out["gemm_vs_parent"]["this_minus_parent_ms"] = round(med(libs["this"]) - med(libs["parent"]), 3)
        out["gemm_vs_parent"]["parent_spread_ms"] = round(max(libs["parent"]) - min(libs["parent"]), 3)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
