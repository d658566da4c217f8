"""Continuing sequences from a start position (LlamaModel.append / admit, sli_model_extend_seqs), timed on ONE model
in ONE process per measurement, in interleaved rounds (wall clock around calls that end in a wait for the stream; the
graphs of every route are captured in a warm-up round). Every figure is a record, not a promise.

  second_turn   Llama-2-7B shapes, batch 1: a 512-token context is prefilled, then a 64-token turn arrives. `append`
                (the GEMM chunks from position 511) against the same 64 tokens teacher-forced through the decode step
                (the prompt buffer forced, 64 advancing steps) and against prefilling all 576 tokens from zero. Each
                round restores the state to (token 511, position 511); rows 0 .. 510 stay valid throughout.
  admission     Llama-3-8B shapes, batch 8: seven sequences decode while a 2048-token prompt is admitted into the
                eighth, whole (one extend call between two decode steps) and by admit(max_tokens=256) with one decode
                step between calls. Per way: the gaps between the completions of consecutive decode steps of the running
                sequences (4 steps before, the admission, 4 steps after), their longest and their median, and the time
                from the admission's start to its end (the chunked way's includes its in-between decode steps).
  no_regression the existing routes against another build's library (--baseline-variant NAME: libsli_NAME.so, the
                parent commit's, built from its tree and copied beside libsli.so): prefill_batch of 8 x 512 tokens
                (Llama-3-8B shapes, batch 8) and the batch-1 512-token prefill, a child process per build in the order
                baseline, this, this, baseline. The bar is the baseline's own round-to-round spread (max - min): the gap
                of the medians has to stay inside it ("inside_baseline_spread").

    python tools/extend_time.py [--rounds 5] [--layers 32] [--baseline-variant NAME] [--only second_turn,...] [--out ...]

Writes profiles/extend_time.json.
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


def _stats(v):
    return {"ms": round(med(v), 3), "ms_rounds": [round(x, 3) for x in v], "spread_ms": round(max(v) - min(v), 3)}


def second_turn(a):
    from simplellminference_amd.model import LlamaModel, preset
    ctx, turn = a.context, a.turn
    cfg = preset("llama2-7b", num_hidden_layers=a.layers, max_length=1024)
    m = LlamaModel(config=cfg, w_dtype=a.weights, kv_dtype=a.kv, seed=1).init()
    assert m.prefill_batch_ok()
    full = _ids(ctx + turn, 0, cfg.vocab_size)
    m.prefill_batch([full[:ctx]])

    def restore():
        m.set_state(full[ctx - 1], ctx - 1, advance=True)

    def append():
        m.append([full[ctx:]])

    def decode():  # the turn through the decode step, teacher-forced from the prompt buffer
        m.set_prompt(full)
        m.set_state(full[ctx - 1], ctx - 1, advance=True)
        for _ in range(turn):
            m.step()

    def from_zero():
        m.prefill_batch([full])

    ms = {"append": [], "decode_steps": [], "prefill_from_zero": []}
    for r in range(-1, a.rounds):  # round -1: the warm-up that captures the graphs
        for k, fn in (("append", append), ("decode_steps", decode), ("prefill_from_zero", from_zero)):
            restore()
            t = _time_ms(fn, m)
            st = m.state()
            assert st["pos"] == ctx + turn - 1 and st["token"] == full[-1] and st["error"] == 0, (k, st)
            if r >= 0:
                ms[k].append(t)
    m.close()
    out = {"model": "llama2-7b", "layers": a.layers, "batch": 1, "context": ctx, "turn": turn,
           **{k: _stats(v) for k, v in ms.items()}}
    ap = med(ms["append"])
    out["decode_over_append"] = round(med(ms["decode_steps"]) / ap, 2)
    out["from_zero_over_append"] = round(med(ms["prefill_from_zero"]) / ap, 2)
    print(f"second turn ({ctx} + {turn}): append {ap:.2f} ms, decode steps {med(ms['decode_steps']):.2f} ms, "
          f"all {ctx + turn} from zero {med(ms['prefill_from_zero']):.2f} ms", flush=True)
    return out


def admission(a):
    from simplellminference_amd.model import LlamaModel, preset
    B, n, chunk = 8, a.admit_tokens, a.admit_chunk
    cfg = preset("llama3-8b", num_hidden_layers=a.layers, max_length=n + 256)
    m = LlamaModel(config=cfg, w_dtype=a.weights, kv_dtype=a.kv, seed=1, batch=B).init()
    running = [_ids(32, b, cfg.vocab_size) for b in range(B - 1)]
    prompt = _ids(n, B - 1, cfg.vocab_size)

    def timeline(way):
        m.prefill_batch(running, seqs=list(range(B - 1)))
        m.set_state_seq(B - 1, 0, 0, advance=False)
        m.sync()
        marks = []

        def step():
            m.step()
            m.sync()
            marks.append(time.perf_counter())

        for _ in range(4):
            step()
        t0 = time.perf_counter()
        if way == "whole":
            m.extend([prompt], seqs=[B - 1], starts=[0])
        else:
            m.admit([prompt], [B - 1], max_tokens=chunk, between=step)
        m.sync()
        total = (time.perf_counter() - t0) * 1e3
        for _ in range(4):
            step()
        st = m.state(B - 1)
        assert st["pos"] == n - 1 + 4 and st["error"] == 0, (way, st)
        gaps = [(y - x) * 1e3 for x, y in zip(marks, marks[1:])]
        return total, max(gaps), med(gaps), len(gaps)

    res = {w: {"admission_ms": [], "longest_gap_ms": [], "median_gap_ms": []} for w in ("whole", "chunked")}
    for r in range(-1, a.rounds):
        for w in ("whole", "chunked"):
            total, longest, median, ngaps = timeline(w)
            if r >= 0:
                res[w]["admission_ms"].append(total)
                res[w]["longest_gap_ms"].append(longest)
                res[w]["median_gap_ms"].append(median)
                res[w]["gaps"] = ngaps
    m.close()
    out = {"model": "llama3-8b", "layers": a.layers, "batch": B, "running": B - 1, "prompt_tokens": n,
           "max_tokens": chunk}
    for w, d in res.items():
        out[w] = {k: (_stats(v) if isinstance(v, list) else v) for k, v in d.items()}
        print(f"admission {w}: total {med(d['admission_ms']):.2f} ms, longest gap {med(d['longest_gap_ms']):.2f} ms, "
              f"median gap {med(d['median_gap_ms']):.2f} ms", flush=True)
    return out


def ab_child(a):
    """prefill_batch of 8 x 512 and the batch-1 512-token prefill of whichever library SLI_LIB_VARIANT names."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("llama3-8b", num_hidden_layers=a.layers, max_length=1024)
    out = {}
    m = LlamaModel(config=cfg, w_dtype=a.weights, kv_dtype=a.kv, seed=1, batch=8).init()
    prompts = [_ids(512, b, cfg.vocab_size) for b in range(8)]
    ms = [_time_ms(lambda: m.prefill_batch(prompts), m) for _ in range(-1, a.rounds)][1:]
    assert all(m.state(b)["pos"] == 511 and m.state(b)["error"] == 0 for b in range(8))
    m.close()
    out["prefill_batch_8x512"] = ms
    m = LlamaModel(config=cfg, w_dtype=a.weights, kv_dtype=a.kv, seed=1).init()
    assert m.prefill_path() == "mfma"
    ids = _ids(512, 0, cfg.vocab_size)
    ms = [_time_ms(lambda: m.prefill(ids), m) for _ in range(-1, a.rounds)][1:]
    assert m.state()["pos"] == 511 and m.state()["error"] == 0
    m.close()
    out["prefill_b1_512"] = ms
    print(json.dumps(out))


def _child(a, variant):
    env = {k: v for k, v in os.environ.items() if k != "SLI_LIB_VARIANT"}
    if variant:
        env["SLI_LIB_VARIANT"] = variant
    cmd = [sys.executable, os.path.abspath(__file__), "--ab-child", "--rounds", str(a.rounds), "--layers", str(a.layers),
           "--weights", a.weights, "--kv", a.kv]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def no_regression(a):
    runs = {"base": [_child(a, a.baseline_variant)], "own": [_child(a, "")]}
    runs["own"].append(_child(a, ""))
    runs["base"].append(_child(a, a.baseline_variant))
    out = {"baseline_variant": a.baseline_variant, "layers": a.layers}
    for key in ("prefill_batch_8x512", "prefill_b1_512"):
        base = [x for r in runs["base"] for x in r[key]]
        own = [x for r in runs["own"] for x in r[key]]
        gap, spread = med(own) - med(base), max(base) - min(base)
        out[key] = {"baseline_ms": round(med(base), 3), "baseline_ms_rounds": [round(x, 3) for x in base],
                    "baseline_spread_ms": round(spread, 3), "this_build_ms": round(med(own), 3),
                    "this_build_ms_rounds": [round(x, 3) for x in own], "gap_ms": round(gap, 3),
                    "inside_baseline_spread": bool(abs(gap) <= spread)}
        print(f"{key}: this build {med(own):.3f} ms, {a.baseline_variant} {med(base):.3f} ms (its spread "
              f"{spread:.3f} ms)", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--weights", default="f16")
    ap.add_argument("--kv", default="f16")
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--turn", type=int, default=64)
    ap.add_argument("--admit-tokens", type=int, default=2048)
    ap.add_argument("--admit-chunk", type=int, default=256)
    ap.add_argument("--baseline-variant", default="")
    ap.add_argument("--only", default="second_turn,admission,no_regression")
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extend_time.json"))
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a)
    if a.rounds < 3:
        ap.error("at least three interleaved rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("extend_time.py needs the GPU: a timing taken anywhere else says nothing")
    only = a.only.split(",")
    out = {"w_dtype": a.weights, "kv_dtype": a.kv, "rounds": a.rounds}
    if "second_turn" in only:
        out["second_turn"] = second_turn(a)
    if "admission" in only:
        out["admission"] = admission(a)
    if "no_regression" in only:
        if a.baseline_variant:
            out["no_regression"] = no_regression(a)
        else:
            out["no_regression"] = "not measured: no --baseline-variant"
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
