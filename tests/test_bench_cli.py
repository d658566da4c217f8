"""bench.py's command line: a plain run reports only the headline (no roofline / greedy / prefill / CPU-baseline
legs, which take runs of their own and sit behind --full), --steps sets the timed steps, and --dump-outputs writes
the last timed step's outputs (logits, greedy next token) as float .npy files that are the same from run to run.
CPU: the option parsing and the dump writer on a stub model. GPU: two plain runs of the tiny GQA shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "greedy_64", "prefill", "cpu_baseline")


def _bench():
    import bench
    return bench


def test_options(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2) and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


class _StubModel:
    def __init__(self, rows, lo, arg):
        self.rows, self.lo, self.arg = rows, lo, arg

    def logits(self):
        return self.rows, self.lo

    def state(self, b=0):
        return {"last_argmax": self.arg[b]}


class _StubDist:
    """all_gather_object of a 2-rank job whose other rank holds the LOWER vocab half (so order matters)."""

    def __init__(self, other):
        self.other = other

    def all_gather_object(self, out, mine):
        out[0], out[1] = mine, self.other


def test_dump_outputs_writes_float_arrays(tmp_path):
    bench = _bench()
    rows = np.arange(12, dtype=np.float32).reshape(2, 6)
    d = str(tmp_path / "one")
    bench.dump_outputs(d, _StubModel(rows, 0, [5, 11]), 2, None, 0, 1)
    assert sorted(os.listdir(d)) == ["logits.npy", "next_token.npy"]
    lg, nt = np.load(os.path.join(d, "logits.npy")), np.load(os.path.join(d, "next_token.npy"))
    assert lg.dtype == np.float32 and np.array_equal(lg, rows)
    assert nt.dtype == np.float64 and nt.tolist() == [5.0, 11.0]
    # batch 1 hands a flat shard over; two ranks' shards are joined in vocab order whatever order they arrive in
    d = str(tmp_path / "two")
    hi, lo = np.array([3., 4., 5.], np.float32), np.array([[0., 1., 2.]], np.float32)
    bench.dump_outputs(d, _StubModel(hi, 3, [4]), 1, _StubDist((0, lo)), 0, 2)
    assert np.load(os.path.join(d, "logits.npy")).tolist() == [[0., 1., 2., 3., 4., 5.]]
    # only rank 0 writes
    d = str(tmp_path / "rank1")
    bench.dump_outputs(d, _StubModel(hi, 3, [4]), 1, _StubDist((0, lo)), 1, 2)
    assert not os.path.exists(d)


def _run(steps, out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--preset", "tiny-gqa", "--ctx", "64", "--settle-ms", "0",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeatable_outputs(gpu, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    da, db = _run(2, a), _run(3, b)
    for d, steps in ((da, 2), (db, 3)):
        assert d["steps"] == steps and d["step_ms"]["n"] == steps and d["full"] is False
        assert d["unit"] == "tokens/s" and d["higher_is_better"] is True and d["dtype"] == "fp16"
        assert d["ms_per_step"] > 0
        # tokens per step / seconds per step (ms_per_step is rounded to 1e-4 ms, the tiny step takes ~0.05 ms)
        assert d["value"] * d["ms_per_step"] / 1e3 == pytest.approx(d["config"]["global_batch"], rel=1e-2)
        assert not any(k in d for k in FULL_ONLY)
    la, lb = np.load(os.path.join(a, "logits.npy")), np.load(os.path.join(b, "logits.npy"))
    ta, tb = np.load(os.path.join(a, "next_token.npy")), np.load(os.path.join(b, "next_token.npy"))
    assert la.dtype == np.float32 and la.shape == (1, 512) and np.isfinite(la).all() and np.abs(la).max() > 0
    assert ta.dtype == np.float64 and ta.shape == (1,) and int(ta[0]) == int(la[0].argmax())
    assert np.array_equal(la, lb) and np.array_equal(ta, tb)  # same arguments apart from the step count: same outputs
