"""The packed GEMM prompt prefill of a batched model (LlamaModel.prefill_batch, sli_model_prefill_seqs) against the
same prompts teacher-forced through the batched decode step (what predict_batch does with a prompt): Llama-3-8B shapes
at batch 8, 8 prompts of 32 / 128 / 512 tokens, both routes on ONE model in ONE process in interleaved rounds (wall
clock around the call and the wait for the stream; the graphs of both routes are captured in a warm-up round).
Reported per prompt length: every round, the median, the per-round spread (max - min) and the ratio of the medians.
The speed-up is a record, not a promise.

The bar: the group table must cost the batch-1 prefill nothing. A child process per build times the batch-1 512-token
prefill (LlamaModel.prefill, with --weights / --kv; MXFP4 under set_prefill("gemm"), an FP8 cache under "gemm-kv8") of
this build's library and of another build's (--baseline-variant NAME: libsli_NAME.so,
the parent commit's built with `python -m simplellminference_amd.build --variant NAME`, as tools/ab_variants.sh loads
them), in the order baseline, this, this, baseline; the gap of the medians has to stay inside the spread (max - min) of
the baseline's own rounds ("inside_baseline_spread").

    python tools/batch_prefill_time.py [--rounds 3] [--layers 32] [--lens 32,128,512] [--baseline-variant NAME] [--out ...]

Writes profiles/batch_prefill_time.json.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

med = lambda v: sorted(v)[len(v) // 2]


def _ids(n, b, vocab):
    return [(1 + 7919 * i + 104729 * b) % vocab for i in range(n)]


def _time_ms(fn, m):
    m.sync()
    t0 = time.perf_counter()
    fn()
    m.sync()
    return (time.perf_counter() - t0) * 1e3


def batch_rounds(a):
    from simplellminference_amd.model import LlamaModel, preset
    B = a.batch
    cfg = preset("llama3-8b", num_hidden_layers=a.layers, max_length=a.ctx)
    m = LlamaModel(config=cfg, w_dtype=a.weights, kv_dtype=a.kv, seed=1, batch=B, mx_batch=a.weights == "mxfp4").init()
    assert m.prefill_batch_ok()
    out = {}
    for n in a.lens:
        prompts = [_ids(n, b, cfg.vocab_size) for b in range(B)]

        def gemm():
            m.prefill_batch(prompts)

        def decode():  # predict_batch's prompt phase: position 0 .. n - 2 through the decode step, teacher-forced
            for b in range(B):
                m.set_prompt_seq(b, prompts[b])
                m.set_state_seq(b, prompts[b][0], 0, advance=True)
            for _ in range(n - 1):
                m.step()

        ms = {"prefill_batch": [], "decode_steps": []}
        for r in range(-1, a.rounds):  # round -1: the warm-up that captures the graphs
            for k, fn in (("prefill_batch", gemm), ("decode_steps", decode)):  # interleaved: the same clocks
                t = _time_ms(fn, m)
                assert all(m.state(b)["pos"] == n - 1 and m.state(b)["error"] == 0 for b in range(B)), (k, n)
                if r >= 0:
                    ms[k].append(t)
        g, d = med(ms["prefill_batch"]), med(ms["decode_steps"])
        out[str(n)] = {k: {"ms": round(med(v), 3), "ms_rounds": [round(x, 3) for x in v],
                           "spread_ms": round(max(v) - min(v), 3)} for k, v in ms.items()}
        out[str(n)]["decode_over_prefill_batch"] = round(d / g, 2)
        out[str(n)]["prompt_tokens_per_s"] = round(B * (n - 1) / (g * 1e-3), 1)
        print(f"{B} x {n} tokens: prefill_batch {g:.2f} ms, decode steps {d:.2f} ms, ratio {d / g:.2f}", flush=True)
    m.close()
    return out


def b1_child(a):
    """The batch-1 512-token prefill of whichever library SLI_LIB_VARIANT names: one JSON line."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama3-8b", num_hidden_layers=a.layers, max_length=a.ctx)
    ids = _ids(a.b1_tokens, 0, cfg.vocab_size)
    m = LlamaModel(config=cfg, w_dtype=a.weights, kv_dtype=a.kv, seed=1).init()
    # where auto keeps the decode step (MXFP4 weights, an FP8 cache), the GEMM prefill is asked for
    if a.kv == "f8":
        m.set_prefill("gemm-kv8")
    elif a.weights == "mxfp4":
        m.set_prefill("gemm")
    assert m.prefill_path() == "mfma"
    ms = []
    for r in range(-1, a.rounds):
        t = _time_ms(lambda: m.prefill(ids), m)
        if r >= 0:
            ms.append(t)
    assert m.state()["error"] == 0
    m.close()
    print(json.dumps({"ms_rounds": ms}))


def _child(a, variant):
    env = {k: v for k, v in os.environ.items() if k != "SLI_LIB_VARIANT"}
    if variant:
        env["SLI_LIB_VARIANT"] = variant
    cmd = [sys.executable, os.path.abspath(__file__), "--b1-child", "--rounds", str(a.b1_rounds), "--layers",
           str(a.layers), "--ctx", str(a.ctx), "--weights", a.weights, "--kv", a.kv, "--b1-tokens", str(a.b1_tokens)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_rounds"]


def b1_ab(a):
    base = _child(a, a.baseline_variant)
    own = _child(a, "")
    own += _child(a, "")
    base += _child(a, a.baseline_variant)
    gap = med(own) - med(base)
    spread = max(base) - min(base)
    out = {"tokens": a.b1_tokens, "baseline_variant": a.baseline_variant,
           "baseline_ms": round(med(base), 3), "baseline_ms_rounds": [round(x, 3) for x in base],
           "baseline_spread_ms": round(spread, 3),
           "this_build_ms": round(med(own), 3), "this_build_ms_rounds": [round(x, 3) for x in own],
           "gap_ms": round(gap, 3), "inside_baseline_spread": bool(abs(gap) <= spread)}
    print(f"batch-1 {a.b1_tokens}-token prefill: this build {med(own):.3f} ms, {a.baseline_variant} {med(base):.3f} ms "
          f"(its spread {spread:.3f} ms)", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--b1-rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--weights", default="f16")
    ap.add_argument("--kv", default="f16")
    ap.add_argument("--lens", default="32,128,512")
    ap.add_argument("--b1-tokens", type=int, default=512)
    ap.add_argument("--baseline-variant", default="")
    ap.add_argument("--b1-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_prefill_time.json"))
    a = ap.parse_args()
    if a.b1_child:
        return b1_child(a)
    if a.rounds < 3:
        ap.error("at least three interleaved rounds")
    a.lens = [int(x) for x in a.lens.split(",")]
    out = {"model": "llama3-8b", "layers": a.layers, "batch": a.batch, "ctx": a.ctx, "w_dtype": a.weights,
           "kv_dtype": a.kv, "rounds": a.rounds}
    if a.baseline_variant:
        out["batch1_prefill_ab"] = b1_ab(a)
    out["prompts"] = batch_rounds(a)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
