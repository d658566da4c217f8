"""Prompt prefill of an int8 Llama-2-7B under set_prefill("gemm") and set_prefill("gemm-i8a8"), one model, one process,
rounds interleaved after warm-up runs that settle the clocks (the manner of tools/mx8_time.py), and the per-launch times
at M = 256 of the four GEMM roles of the integer-MFMA body and of the two quantisers.

    python tools/i8a8_time.py [--layers 32] [--tokens 512] [--rounds 5] [--reps 4] [--out profiles/i8a8_prefill.json]

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

from tools.mx8_time import _launch_us  # noqa: E402  (n launches in one graph, replayed between events)


def launches(torch, cfg, M=256):
    """One launch each at the 7B shapes, weights and activations random codes (timing only). The operands of one launch
    stay resident between replays; tools/pgemm_i8a8_lab times the GEMMs with the weights streamed from HBM."""
    from simplellminference_amd import ops
    D, I, hq, hkv, hd = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    i8 = lambda *s: torch.randint(-127, 128, s, device="cuda", dtype=torch.int8)
    W = lambda n, k: (i8(n, k), torch.full((n,), 2.0 ** -9, device="cuda"))
    A = lambda k: (i8(M, k), torch.full((M,), 2.0 ** -6, device="cuda"))
    T = M + 16
    sin_t, cos_t = ops.rope_cache(hd, T, 10000.0)
    q, y = torch.empty(M, hq * hd, device="cuda"), torch.zeros(M, D, device="cuda")
    kc = torch.empty(hkv, T, hd, device="cuda", dtype=torch.float16)
    vc, ahi = torch.empty_like(kc), torch.zeros(M, I, device="cuda", dtype=torch.float16)
    alo, x = torch.zeros_like(ahi), torch.randn(M, D, device="cuda")
    wn = torch.ones(D, device="cuda")
    qkv, gu, wo, down, lm = W((hq + 2 * hkv) * hd, D), W(2 * I, D), W(D, hq * hd), W(D, I), W(cfg.vocab_size, D)
    aD, aQ, aI = A(D), A(hq * hd), A(I)
    logits = torch.empty(M, cfg.vocab_size, device="cuda")
    return {
        "qkv": _launch_us(torch, lambda: ops.prefill_gemm_qkv_i8a8(*qkv, *aD, q, kc, vc, sin_t, cos_t, hq, hkv, hd, 0, M)),
        "gate_up": _launch_us(torch, lambda: ops.prefill_gemm_gate_up_i8a8(*gu, *aD, ahi, alo)),
        "wo": _launch_us(torch, lambda: ops.prefill_gemm_resid_i8a8(*wo, *aQ, y, resid=y)),
        "down": _launch_us(torch, lambda: ops.prefill_gemm_resid_i8a8(*down, *aI, y, resid=y)),
        "logits": _launch_us(torch, lambda: ops.prefill_gemm_logits_i8a8(*lm, *aD, logits)),
        "norm_quant": _launch_us(torch, lambda: ops.prefill_norm_quant_i8(x, wn, 1e-5)),
        "pair_quant_inter": _launch_us(torch, lambda: ops.prefill_quant_i8(ahi, alo)),
    }


def _model(a):
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama2-7b", num_hidden_layers=a.layers, max_length=a.tokens + 16)
    prompt = [(1 + 7919 * i) % cfg.vocab_size for i in range(a.tokens)]
    return cfg, LlamaModel(config=cfg, w_dtype="i8", kv_dtype="f16", seed=1).init(), prompt


def _once(m, prompt, mode, reps):
    m.set_prefill(mode)
    m.reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        m.prefill(prompt)  # returns after the stream has been waited for
    return (time.perf_counter() - t0) / reps * 1e3


def gemm_ms(a):
    """ms of the third round of `reps` prefills under "gemm" (two warm-up rounds): a child process's whole job."""
    _, m, prompt = _model(a)
    out = [_once(m, prompt, "gemm", a.reps) for _ in range(3)]
    m.close()
    return out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8a8_prefill.json"))
    ap.add_argument("--parent-variant", default="", help="libsli_<name>.so built from the parent commit: also time "
                    '"gemm" under this library and that one, a fresh process each, rounds interleaved')
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps({"ms": gemm_ms(a)}))
        return
    import torch
    cfg, m, prompt = _model(a)
    modes = ("gemm", "gemm-i8a8")
    for mode in modes * 2:  # graphs captured, clocks settled
        _once(m, prompt, mode, a.reps)
    ms = {mode: [] for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            ms[mode].append(_once(m, prompt, mode, a.reps))
    m.close()
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"model": "llama2-7b", "w_dtype": "i8", "layers": a.layers, "tokens": a.tokens, "rounds": a.rounds, "reps": a.reps}
    for mode in modes:
        out[mode] = {"ms": round(med(ms[mode]), 3), "ms_rounds": [round(v, 3) for v in ms[mode]],
                     "tok_s": round((a.tokens - 1) / med(ms[mode]) * 1e3, 1)}
    out["time_ratio_i8a8_over_gemm"] = round(out["gemm-i8a8"]["ms"] / out["gemm"]["ms"], 4)
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
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True, timeout=300)
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
