"""Prefix copy between the sequences of a K/V cache (csrc/kv_copy.h: sli_kv_copy_prefix / ops.kv_copy_prefix on caller
buffers, sli_model_copy_prefix / LlamaModel.fork on a model's own cache).

Op level: a byte copy, so the bar is byte equality: dst rows [0, n) equal src's, every other byte of both caches is
unchanged. Model level: a forked sequence continued with append decodes as the oracle does on the concatenated list
(tokens bit-equal, logits within 1e-3: the bars of tests/test_gpu_batch_prefill.py). Weight seed 20 from
tests/extend_scenarios.py ("fork": minimum top-2 gap 1.1e-2 over the compared positions; seed 0: 2.6e-5).
"""
import numpy as np
import pytest

from tests import extend_scenarios as S

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 2, 40, 64)  # [L][B][hkv][T][hd]


@pytest.mark.parametrize("n", [0, 1, 33, 40])
@pytest.mark.parametrize("dtype", ["uint8", "float16", "float32"])
def test_op_copies_the_prefix_and_nothing_else(gpu, dtype, n):
    from simplellminference_amd import ops
    torch = gpu
    r = np.random.default_rng(40 * n + len(dtype))
    nbytes = int(np.prod(SHAPE)) * np.dtype(dtype).itemsize
    raw = [r.integers(0, 256, nbytes, dtype=np.uint8) for _ in range(2)]  # every byte pattern, NaN codes included
    k0, v0 = (torch.from_numpy(a).cuda() for a in raw)
    tdt = getattr(torch, dtype)
    kc, vc = k0.clone().view(tdt).view(SHAPE), v0.clone().view(tdt).view(SHAPE)
    src, dst = 2, 0
    ops.kv_copy_prefix(kc, vc, src, dst, n)
    torch.cuda.synchronize()
    for got, was in ((kc, k0), (vc, v0)):
        got = got.view(-1).view(torch.uint8).cpu().numpy().reshape(*SHAPE[:4], -1)
        want = was.cpu().numpy().reshape(*SHAPE[:4], -1).copy()
        want[:, dst, :, :n] = want[:, src, :, :n]
        assert np.array_equal(got, want)


def test_op_refusals(gpu):
    from simplellminference_amd import ops
    from simplellminference_amd._lib import SliError
    torch = gpu
    kc = torch.zeros(SHAPE, dtype=torch.float16, device="cuda")
    vc = torch.zeros(SHAPE, dtype=torch.float16, device="cuda")
    for src, dst, n in ((1, 1, 4), (3, 0, 4), (0, -1, 4), (0, 1, 41), (0, 1, -1)):
        with pytest.raises(SliError):
            ops.kv_copy_prefix(kc, vc, src, dst, n)
    small = torch.zeros((2, 3, 2, 40, 16), dtype=torch.float16, device="cuda")  # a 32-byte row
    with pytest.raises(SliError):
        ops.kv_copy_prefix(small, small.clone(), 0, 1, 4)
    with pytest.raises(ValueError):
        ops.kv_copy_prefix(kc, vc.float(), 0, 1, 4)


def test_fork_then_append_matches_oracle(gpu, oracle):
    """fork(0, 1, 20) after a 30-token prefill, then 7 tokens appended to sequence 1: the oracle's run on p[:21] + the
    7 tokens. Sequence 0 is untouched and decodes on as the oracle does on p."""
    from simplellminference_amd.model import LlamaModel, preset
    cfg = preset("tiny-gqa")
    seed = S.SEEDS["fork"]
    (p, forced), first = S.fork(oracle, cfg, seed)
    L = cfg.num_hidden_layers
    gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=seed, batch=3).init()
    gm.prefill_batch([p, S.prompt(9, cfg.vocab_size, seed=8)], seqs=[0, 2])
    snap = lambda b: ([gm.kv(layer, which, 64, seq=b) for layer in range(L) for which in (0, 1)], gm.state(b),
                      gm.history(b, 64))
    before = {b: snap(b) for b in (0, 1, 2)}
    gm.fork(0, 1, 20)
    after = {b: snap(b) for b in (0, 1, 2)}
    for b in (0, 2):  # src and the bystander: rows, state and history as they were
        assert all(np.array_equal(x, y) for x, y in zip(before[b][0], after[b][0])), b
        assert before[b][1] == after[b][1] and np.array_equal(before[b][2], after[b][2]), b
    for x0, x1, y in zip(before[1][0], after[1][0], after[0][0]):
        assert np.array_equal(x1[:20], y[:20]) and np.array_equal(x1[20:], x0[20:])
    st = gm.state(1)
    assert (st["pos"], st["token"]) == (20, p[20]) and np.array_equal(gm.history(1, 21), p[:21])
    gm.step()  # dst waits: a step does not move it
    gm.sync()
    assert gm.state(1)["pos"] == 20 and gm.state(0)["pos"] == 30
    gm.append([forced[21:]], seqs=[1])
    assert gm.state(1)["pos"] == len(forced) - 1
    rec = [{} for _ in range(3)]
    for _ in range(64 - len(forced) + 1):
        pos = [gm.state(b)["pos"] for b in range(3)]
        gm.step()
        lg = gm.logits()[0]
        for b in range(3):
            rec[b][pos[b]] = lg[b].copy()
    gm.sync()
    hist = [gm.history(b, 64) for b in range(2)]
    gm.close()
    for b, lst in enumerate((p, forced)):
        otok, olog, _ = S.run(oracle, cfg, lst, 64, seed)
        assert np.array_equal(hist[b], otok), b
        ps = sorted(t for t in rec[b] if t >= max(first[b], len(lst) - 1))
        err = max(float(np.abs(rec[b][t] - olog[t]).max()) for t in ps)
        print(f"sequence {b}: {len(ps)} positions, max|dlogit| {err:.3e}")
        assert err <= 1e-3, (b, err)


def test_fork_default_and_group(gpu):
    """n defaults to src's position; a TP group copies every rank's shard."""
    from simplellminference_amd.model import LlamaModel, TPGroup, preset
    cfg = preset("tiny-gqa")
    gm = LlamaModel(config=cfg, w_dtype="f16", kv_dtype="f16", seed=0, batch=2).init()
    p = S.prompt(12, cfg.vocab_size)
    gm.prefill_batch([p], seqs=[1])
    gm.fork(1, 0)
    assert gm.state(0)["pos"] == 11 and gm.state(0)["token"] == p[11]
    assert np.array_equal(gm.kv(1, 1, 11, seq=0), gm.kv(1, 1, 11, seq=1))
    gm.close()
    g = TPGroup(preset("tiny-h8"), 2, w_dtype="f16", kv_dtype="f16", seed=0, batch=2).init()
    g.predict_batch([p, p[:3]], 14)
    g.fork(0, 1, 9)
    for m in g.ranks:
        assert m.state(1)["pos"] == 9 and m.state(1)["token"] == p[9]
        assert np.array_equal(m.kv(0, 0, 9, seq=1), m.kv(0, 0, 9, seq=0))
    g.close()
