"""What scoring costs (LlamaModel.score, sli_model_score_seqs) beside the packed GEMM prefill it rides on, and beside
today's route to the same numbers (the prompt teacher-forced through the decode step with want_logits and a numpy
log-softmax on the host). One child process per configuration:

    llama3-8b shapes at batch 8, 8 prompts of 512 tokens;   llama2-7b shapes at batch 1, 1 prompt of 512 tokens

synthetic weights, every shape warmed in a round that is not reported, then at least three interleaved rounds of
  (a) prefill_batch   (b) score   (c) predict_batch / predict with want_logits, then the numpy log-softmax
(wall clock around the call and the wait for the stream). Reported per configuration: every round, the medians,
(b) - (a) = the LM head plus the score launch of all chunks, (c) / (b), and, one launch at a time through the
kernel-level entries on the configuration's own shapes (HIP events, the median of --launch-iters launches of a 256-row
chunk): the LM-head GEMM (role 3) with its algorithmic flops over its time and the bound that applies (the larger of
flops over the MFMA peak and bytes over the HBM peak; peaks: MI355X spec, 2.5 PFLOP/s dense fp16 MFMA, 8 TB/s), and
the score launch against a plain read of the same M * V * 4 bytes (torch's sum over the buffer).
Nothing here is a promise: the numbers are a record of one session.

    python tools/score_time.py [--rounds 3] [--layers 32] [--tokens 512] [--weights f16] [--out ...]

Writes profiles/score_time.json.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12  # MI355X spec: dense fp16 MFMA, HBM3E
CONFIGS = {"llama3-8b": 8, "llama2-7b": 1}  # preset -> batch
med = lambda v: sorted(v)[len(v) // 2]


def _ids(n, b, vocab):
    return [(1 + 7919 * i + 104729 * b) % vocab for i in range(n)]


def _time_ms(fn, m):
    m.sync()
    t0 = time.perf_counter()
    r = fn()
    m.sync()
    return (time.perf_counter() - t0) * 1e3, r


def _log_softmax_rows(logits, targets):
    """numpy, fp32: log-probability of targets[t] under row t (today's host-side scoring)."""
    import numpy as np
    mx = logits.max(-1)
    lse = mx + np.log(np.exp(logits - mx[:, None]).sum(-1))
    return logits[np.arange(len(targets)), targets] - lse


def _launches(a, cfg):
    """The LM-head GEMM, the score launch and a plain read, one 256-row chunk each, by HIP events."""
    import torch
    from simplellminference_amd import ops
    V, D, M = cfg.vocab_size, cfg.hidden_size, 256
    g = torch.Generator(device="cuda").manual_seed(1)
    w32 = torch.randn(V, D, device="cuda", generator=g) / D ** 0.5
    x = torch.randn(M, D, device="cuda", generator=g)
    hi, lo = ops.prefill_norm_split(x, None, 1e-5)
    kw, wbytes = {}, 2.0
    if a.weights == "f16":
        w = w32.half()
    elif a.weights == "i8":
        s = w32.abs().amax(1) / 127
        w, kw, wbytes = (w32 / s[:, None]).round().clamp(-127, 127).to(torch.int8), dict(row_scale=s.contiguous()), 1.0
    else:
        w, sc = ops.quant_mxfp4(w32)
        kw, wbytes = dict(scales=sc), 0.5 + 1 / 32
    del w32
    ld = (V + 3) // 4 * 4
    y = torch.empty(M, ld, device="cuda")
    t = torch.randint(0, V, (M,), device="cuda", dtype=torch.int32)

    def ev(fn):
        ms = []
        for i in range(-2, a.launch_iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 0:
                ms.append(e0.elapsed_time(e1))
        return med(ms)

    tiling = ops.prefill_gemm_logits(w, hi, lo, y, **kw)
    lm = ev(lambda: ops.prefill_gemm_logits(w, hi, lo, y, **kw))
    sc_ms = ev(lambda: ops.score_rows(y[:, :V], t))
    rd = ev(lambda: y.sum())
    flops = 2.0 * M * V * D
    nbytes = V * D * wbytes + M * D * 4 + M * V * 4  # the table once, the hi / lo rows, the logits written
    t_f, t_b = flops / PEAK_FLOPS * 1e3, nbytes / PEAK_BYTES * 1e3
    return {"chunk_rows": M, "tiling": tiling,
            "lm_head_ms": round(lm, 4), "lm_head_tflops": round(flops / (lm * 1e-3) / 1e12, 1),
            "lm_head_flops_floor_ms": round(t_f, 4), "lm_head_bytes_floor_ms": round(t_b, 4),
            "lm_head_bound": "flops" if t_f >= t_b else "bytes", "lm_head_share_of_bound": round(max(t_f, t_b) / lm, 3),
            "score_ms": round(sc_ms, 4), "score_bytes": M * V * 4, "score_gb_per_s": round(M * V * 4 / (sc_ms * 1e-3) / 1e9, 1),
            "plain_read_ms": round(rd, 4), "plain_read_gb_per_s": round(M * V * 4 / (rd * 1e-3) / 1e9, 1),
            "score_over_plain_read": round(sc_ms / rd, 2)}


def child(a):
    # torch before the library (as tests/conftest.py and bench.py load them, and tools/kv8_time.py explains): the torch
    # wheel bundles a ROCm runtime under the system runtime's sonames, and whichever is loaded first serves the process
    import torch  # noqa: F401
    import numpy as np
    from simplellminference_amd.model import LlamaModel, preset
    B, n = CONFIGS[a.child], a.tokens
    cfg = preset(a.child, num_hidden_layers=a.layers, max_length=a.ctx)
    m = LlamaModel(config=cfg, w_dtype=a.weights, kv_dtype=a.kv, seed=1, batch=B, mx_batch=a.weights == "mxfp4" and B > 1).init()
    assert m.score_ok()
    prompts = [_ids(n, b, cfg.vocab_size) for b in range(B)]
    host = {"forward_ms": [], "log_softmax_ms": []}

    def route_c():
        t0 = time.perf_counter()
        if B > 1:
            _, logits = m.predict_batch(prompts, n, want_logits=True)
        else:
            _, logits = m.predict(prompts[0], n, want_logits=True)
            logits = logits[None]
        t1 = time.perf_counter()
        out = [_log_softmax_rows(logits[b, :n - 1], np.asarray(prompts[b][1:])) for b in range(B)]
        host["forward_ms"].append((t1 - t0) * 1e3)
        host["log_softmax_ms"].append((time.perf_counter() - t1) * 1e3)
        return out

    routes = (("prefill_batch", lambda: m.prefill_batch(prompts)), ("score", lambda: m.score(prompts)),
              ("decode_logits_numpy", route_c))
    ms = {k: [] for k, _ in routes}
    got = {}
    for r in range(-1, a.rounds):  # round -1: the warm-up that captures the graphs and allocates the scratch
        # an untimed prefill first: (a) would otherwise always start behind (c)'s seconds of host work, on a chip that
        # has idled (measured so at batch 1: (a) 1.3 ms SLOWER than (b))
        m.reset()
        m.prefill_batch(prompts)
        for k, fn in routes:
            m.reset()
            t, res = _time_ms(fn, m)
            if r >= 0:
                ms[k].append(t)
            got[k] = res
    for k in host:
        host[k] = host[k][1:]
    # the two routes score the same tokens (the project's 2e-3 bar between the GEMM prefill and the decode step)
    dmax = max(float(np.abs(got["score"][b]["logprobs"] - got["decode_logits_numpy"][b]).max()) for b in range(B))
    lp = np.concatenate([got["score"][b]["logprobs"] for b in range(B)]).astype(np.float64)
    m.close()
    a_ms, b_ms, c_ms = (med(ms[k]) for k, _ in routes)
    rows = B * (n - 1)
    out = {"model": a.child, "layers": a.layers, "batch": B, "tokens": n, "w_dtype": a.weights, "kv_dtype": a.kv,
           "rounds": a.rounds, "scored_positions": rows,
           "routes": {k: {"ms": round(med(v), 3), "ms_rounds": [round(x, 3) for x in v],
                          "spread_ms": round(max(v) - min(v), 3)} for k, v in ms.items()},
           "decode_route_host": {k: round(med(v), 3) for k, v in host.items()},
           "score_minus_prefill_ms": round(b_ms - a_ms, 3),
           "score_over_prefill": round(b_ms / a_ms, 3),
           "decode_route_over_score": round(c_ms / b_ms, 2),
           "lm_head_flops_all_chunks": 2.0 * rows * cfg.vocab_size * cfg.hidden_size,
           "max_abs_dlogprob_between_routes": dmax, "mean_nll": float(-lp.mean()),
           "launches": _launches(a, cfg)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--weights", default="f16")
    ap.add_argument("--kv", default="f16")
    ap.add_argument("--launch-iters", type=int, default=9)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_time.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.rounds < 3:
        ap.error("at least three interleaved rounds")
    out = {"peaks": {"fp16_mfma_flops": PEAK_FLOPS, "hbm_bytes_per_s": PEAK_BYTES, "source": "MI355X spec"}, "configs": []}
    for name in a.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(a.rounds), "--layers",
               str(a.layers), "--tokens", str(a.tokens), "--ctx", str(a.ctx), "--weights", a.weights, "--kv", a.kv,
               "--launch-iters", str(a.launch_iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"{name}: child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        c = json.loads(r.stdout.strip().splitlines()[-1])
        out["configs"].append(c)
        L = c["launches"]
        print(f"{name} batch {c['batch']} x {c['tokens']}: prefill_batch {c['routes']['prefill_batch']['ms']:.1f} ms, "
              f"score {c['routes']['score']['ms']:.1f} ms (+{c['score_minus_prefill_ms']:.1f}), decode route "
              f"{c['routes']['decode_logits_numpy']['ms']:.1f} ms ({c['decode_route_over_score']:.1f}x); per chunk: LM head "
              f"{L['lm_head_ms']:.3f} ms ({L['lm_head_tflops']:.0f} TFLOP/s, {L['lm_head_bound']}-bound floor), score "
              f"{L['score_ms']:.3f} ms vs plain read {L['plain_read_ms']:.3f} ms", flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
