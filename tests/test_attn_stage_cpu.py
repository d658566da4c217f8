"""sli_decode_attn (include/sli.h "decode stages, for tests and labs") without a GPU: the symbols, every refusal with its
message (no call here would pass the checks, so nothing reaches a device), the launch geometry of production models
reproduced by sli_decode_attn_plan at 256 compute units, and the coverage condition of the GPU file's cells."""
import ctypes

import pytest

from simplellminference_amd import _lib, ops
from tests import attn_ref as R

A = 0x10000  # a 16-byte aligned address that is never dereferenced: every call below is refused on the host


def test_symbols():
    lib = _lib.load()
    for name in ("sli_decode_attn", "sli_decode_attn_plan"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()


def _call(cus=256, plan_only=False, **kw):
    f = dict(q=A, k=A, v=A, kv_dtype=_lib.DT_F16, out=A, part=A, counters=A, pos=A, pos_seq_stride=6, B=4, hq=8, hkv=2,
             hd=128, T=1024, merge=2)
    f.update(kw)
    a, p = _lib.AttnLaunch(**f), _lib.AttnPlan(cus=cus)
    lib = _lib.load()
    rc = lib.sli_decode_attn_plan(ctypes.byref(a), ctypes.byref(p)) if plan_only else \
        lib.sli_decode_attn(ctypes.byref(a), ctypes.byref(p), None)
    return rc, (lib.sli_last_error() or b"").decode()


ARG, SHAPE = 1, 2
REFUSALS = [
    ("null q", lambda: _call(q=None), ARG, "null pointer"),
    ("null cache", lambda: _call(v=None), ARG, "null pointer"),
    ("null out", lambda: _call(out=None), ARG, "null pointer"),
    ("null partials", lambda: _call(part=None), ARG, "null pointer"),
    ("null counters", lambda: _call(counters=None), ARG, "null pointer"),
    ("null position", lambda: _call(pos=None), ARG, "null pointer"),
    ("misaligned q", lambda: _call(q=A + 4), ARG, "16-byte alignment"),
    ("misaligned k", lambda: _call(k=A + 8), ARG, "16-byte alignment"),
    ("misaligned v", lambda: _call(v=A + 2), ARG, "16-byte alignment"),
    ("misaligned out", lambda: _call(out=A + 4), ARG, "16-byte alignment"),
    ("misaligned partials", lambda: _call(part=A + 8), ARG, "16-byte alignment"),
    ("misaligned position", lambda: _call(pos=A + 2), ARG, "4-byte aligned"),
    ("kv dtype", lambda: _call(kv_dtype=_lib.DT_I8), ARG, "bad kv dtype"),
    ("head_dim", lambda: _call(hd=96), SHAPE, "head_dim must be 64 or 128"),
    ("hq % hkv", lambda: _call(hq=7), SHAPE, "hq must be a multiple of hkv"),
    ("heads per kv head", lambda: _call(hq=6), SHAPE, "heads per kv head must be 1, 2, 4 or 8"),
    ("sixteen heads per kv head", lambda: _call(hq=32), SHAPE, "heads per kv head must be 1, 2, 4 or 8"),
    ("B = 0", lambda: _call(B=0), SHAPE, "B must be 1 .. 8"),
    ("B = 9", lambda: _call(B=9), SHAPE, "B must be 1 .. 8"),
    ("T = 0", lambda: _call(T=0), SHAPE, "T must be positive"),
    ("position stride", lambda: _call(pos_seq_stride=0), ARG, "pos_seq_stride must be >= 1"),
    ("merge = 3", lambda: _call(merge=3), ARG, "merge must be 0"),
    ("merge = -1", lambda: _call(merge=-1), ARG, "merge must be 0"),
    ("FP8 with the consumer's merge", lambda: _call(kv_dtype=_lib.DT_F8E4M3, merge=1), ARG,
     "an FP8 cache takes no merge in the consumer"),
    # (cus between the device's count and 4096 needs a device to refuse: tests/test_gpu_decode_attn.py)
    ("cus above 4096", lambda: _call(cus=100000), ARG, "cus exceeds"),
    ("cus above 4096, the plan", lambda: _call(plan_only=True, cus=4097), ARG, "cus exceeds"),
    ("hq above 4096", lambda: _call(hq=8192, hkv=8192), SHAPE, "hq exceeds 4096"),
    ("a layer of 2^31 elements", lambda: _call(B=8, hq=4096, hkv=4096, T=512), SHAPE, "below 2^31 elements"),
    ("misaligned counters", lambda: _call(counters=A + 2), ARG, "4-byte aligned"),
    ("negative cus", lambda: _call(cus=-1), ARG, "cus must be"),
    ("fp32 splits beyond the merge", lambda: _call(kv_dtype=_lib.DT_F32, T=129 * 128), SHAPE, "context too long"),
    ("the plan refuses the same", lambda: _call(plan_only=True, hd=96), SHAPE, "head_dim must be 64 or 128"),
    ("the plan's splits", lambda: _call(plan_only=True, kv_dtype=_lib.DT_F32, T=129 * 128), SHAPE, "context too long"),
]


@pytest.mark.parametrize("what,fn,code,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, fn, code, msg):
    rc, err = fn()
    assert rc == code, (what, rc, err)
    assert msg in err, (what, err)


def test_batch_1_ignores_the_position_stride():
    rc, err = _call(plan_only=True, B=1, pos_seq_stride=0)
    assert rc == 0, err


def _plan(kv, B, hq, hkv, hd, T, merge, cus=256):
    return ops.decode_attn_plan(R.DT[kv], B, hq, hkv, hd, T, merge=merge, cus=cus)


def test_geometry_facts():
    """Hand-checked against attention.h's AttnGeom / attn_waves and attn_mfma.h's attn_mfma_tpw."""
    # fp16, hd 128, batch 1, the merge left to the consumer: register-staged, 16 B = 8 halves per lane, 16 lanes per row,
    # 4 rows per instruction x 64 slots = 256 positions per workgroup, 16 waves (MHA)
    p = _plan("f16", 1, 32, 32, 128, 2048, 1)
    assert (p["kernel"], p["ppwg"], p["waves"], p["g"], p["kv_group"], p["max_splits"], p["grid"], p["merge_grid"],
            p["merge"], p["tpw"], p["nbuf"]) == (0, 256, 16, 1, 1, 8, 256, 0, 1, 0, 0)
    # Llama-3-8B batch 1 (DESIGN: "8 kv heads x 16 splits = 128 workgroups" after the split into two GQA-2 groups)
    p = _plan("f16", 1, 32, 8, 128, 2048, 1)
    assert (p["kernel"], p["g"], p["kv_group"], p["waves"], p["max_splits"], p["grid"]) == (0, 2, 2, 16, 8, 128)
    # ... and unsplit where the doubled grid would not fit the chip
    p = _plan("f16", 1, 32, 8, 128, 2048, 1, cus=127)
    assert (p["g"], p["kv_group"], p["waves"], p["grid"]) == (4, 1, 8, 64)
    # fp32, hd 128: 4 floats per lane, 2 rows per instruction: 128 positions; a merge launch of one thread per output
    p = _plan("f32", 8, 32, 8, 128, 4096, 2)
    assert (p["kernel"], p["ppwg"], p["g"], p["kv_group"], p["waves"], p["max_splits"], p["grid"], p["merge_grid"],
            p["merge"]) == (0, 128, 4, 1, 8, 32, 64 * 32, 64 * 2, 2)
    assert _plan("f32", 1, 2, 2, 64, 1024, 0)["ppwg"] == 256 and _plan("f16", 1, 2, 2, 64, 1024, 1)["ppwg"] == 512
    assert _plan("f32", 1, 16, 2, 128, 1024, 0)["waves"] == 4  # GQA-8
    # MFMA: Llama-3-8B at batch 8 (64 kv heads), T 4096: 1024 keys per CU = 8 tiles per wave, 4 splits, one workgroup
    # per CU; the requested merge launch becomes the in-launch merge
    p = _plan("f16", 8, 32, 8, 128, 4096, 2)
    assert (p["kernel"], p["tpw"], p["nbuf"], p["ppwg"], p["max_splits"], p["grid"], p["merge"], p["merge_grid"],
            p["waves"]) == (1, 8, 2, 1024, 4, 256, 0, 0, 4)
    # the TP-8 shard: "8 kv heads, ctx 4096 at 16 splits on 128 workgroups" (attn_mfma.h) is the batch-2 shard;
    # never more than 16 splits
    p = _plan("f16", 2, 4, 4, 128, 4096, 2)
    assert (p["tpw"], p["max_splits"], p["grid"]) == (2, 16, 128)
    # hd 64: never a split shorter than the partial buffer's 256 positions
    assert _plan("f8", 1, 2, 2, 64, 1024, 0)["tpw"] == 2
    assert _plan("f8", 1, 4, 4, 128, 2048, 0)["nbuf"] == 1


def _cell_plans():
    out = []
    for c in R.CELLS:
        p = _plan(c["kv"], c["B"], c["hq"], c["hkv"], c["hd"], c["T"], c["merge"], cus=c["cus"] or 256)
        out.append((c, p))
    return out


def test_cells_are_small():
    for c in R.CELLS:
        assert c["T"] <= 4352 and c["B"] * c["hkv"] <= 16 and c["T"] % 8 == 0, c


def test_cells_cover_production():
    """The geometry class of the attention launch of every production model, with every cache type at T 2048 and 4096,
    is the class of a cell the GPU file runs."""
    have = {R.plan_class(c["kv"], c["hd"], p) for c, p in _cell_plans()}
    missing = []
    for kv, B, hq, hkv, hd, T, merge in R.production_launches():
        cl = R.plan_class(kv, hd, _plan(kv, B, hq, hkv, hd, T, merge))
        if cl not in have:
            missing.append(((kv, B, hq, hkv, hd, T, merge), cl))
    assert not missing, missing


def test_cells_take_the_listed_branches():
    cp = _cell_plans()

    def some(pred):
        return any(pred(c, p) for c, p in cp)
    for kv in ("f16", "f32"):  # R1
        for hd in (64, 128):
            for g in (1, 2):
                assert some(lambda c, p: (c["kv"], c["hd"], p["g"], p["kernel"], p["merge"], c["B"], p["max_splits"]) ==
                            (kv, hd, g, 0, 1, 1, 4))
    assert some(lambda c, p: c["name"] == "R2" and p["kv_group"] == 2 and p["g"] == 2)
    assert some(lambda c, p: c["name"] == "R2" and p["kv_group"] == 1 and p["g"] == 4 and p["waves"] == 8)
    assert some(lambda c, p: c["name"] == "R2" and p["g"] == 8 and p["waves"] == 4)
    for g in (1, 2, 4, 8):  # R3: the merge launch at a batch
        assert some(lambda c, p: c["name"] == "R3" and c["B"] == 4 and p["g"] == g and p["kv_group"] == 1 and
                    p["merge"] == 2 and p["merge_grid"] > 0)
    assert some(lambda c, p: c["name"] == "R3" and p["kv_group"] == 2 and p["merge_grid"] > 0)
    assert some(lambda c, p: c["name"] == "R3" and p["max_splits"] == 17)
    for c, p in cp:
        if c["name"] in ("M1", "M2"):  # the requested merge launch became the in-launch merge
            assert (p["kernel"], p["merge"], p["merge_grid"], p["kv_group"]) == (1, 0, 0, 1), (c, p)
        if c["name"] == "M3":
            assert (p["kernel"], p["merge"]) == (1, 0)
        if c["name"] in ("R1", "R2", "R3", "R4"):
            assert p["kernel"] == 0 and p["merge"] == c["merge"], (c, p)
    for kv in ("f16", "f8"):  # every MFMA instantiation (hd, G, ring slots) and the refilled ring
        for hd in (64, 128):
            for g in (1, 2, 4, 8):
                for nbuf, refill in ((2, False), (2, True)) + (((1, False),) if hd == 128 else ()):
                    assert some(lambda c, p: (c["kv"], c["hd"], p["g"], p["nbuf"], p["tpw"] > p["nbuf"], p["kernel"]) ==
                                (kv, hd, g, nbuf, refill, 1)), (kv, hd, g, nbuf, refill)


def test_needle_rows_reach_every_class_in_every_cell():
    """The needle builder's claim, without a GPU: over the position vectors the GPU file runs, every class of needle row
    (row 0, pos, first / last row of a wave slice, of a tile, of a split) is hit in every cell."""
    for c, p in _cell_plans():
        hits = {}
        for i, pos in enumerate(R.cell_sets(c, p, "needle")):
            R.needle(pos, c["hq"], c["hkv"], c["hd"], c["T"], c["kv"], p, i, hits)
        assert set(hits) == set(R.NEEDLE_CLASSES), (R.cell_id(c), hits)


def test_every_cell_runs_every_listed_position():
    """Over the needle and the uniform family's position vectors, every cell runs every position of the issue's list
    that its T admits (0, a slice minus 1, a slice, 31, 32, ppwg - 1, ppwg, the odd one of the last split, T - 1); a
    batch has a sequence at 0 between two at T - 1; the 17-split cells run 17, 16 and 1 live splits."""
    for c, p in _cell_plans():
        want = set(R.positions(p, c["T"]))
        sl, last = p["ppwg"] // p["waves"], (p["max_splits"] - 1) * p["ppwg"]
        listed = {x for x in (0, sl - 1, sl, 31, 32, p["ppwg"] - 1, p["ppwg"], c["T"] - 1) if x < c["T"]}
        assert want >= listed and len(want - listed) <= 1 and all(last <= x < c["T"] - 1 for x in want - listed), R.cell_id(c)
        ran = {x for f in ("needle", "uniform") for v in R.cell_sets(c, p, f) for x in v}
        assert ran >= want, (R.cell_id(c), sorted(want - ran))
        for f in ("needle", "uniform", "real"):
            sets = R.cell_sets(c, p, f)
            assert all(len(v) == c["B"] and all(0 <= x < c["T"] for x in v) for v in sets)
            if c["B"] >= 3:
                assert sets[0][:3] == [c["T"] - 1, 0, c["T"] - 1]
            if c.get("splits17"):
                assert sorted(R.ns_of_heads(sets[-1], 1, p).tolist()) == [1, 16, 17, 17]


def test_split_length_table():
    """attn_ref.PPWG_CACHE (the rule of production_merge and the R1 cells' T) is the register-staged kernel's own split."""
    for (kv, hd), ppwg in R.PPWG_CACHE.items():
        p = _plan(kv, 1, 2, 2, hd, 4 * ppwg, 1)
        assert (p["kernel"], p["ppwg"], p["max_splits"]) == (0, ppwg, 4), (kv, hd, p)
    assert R.PRODUCTION == (("llama2-7b", 1, 1), ("llama2-7b", 4, 1), ("llama2-7b", 8, 1), ("llama3-8b", 1, 1),
                            ("llama3-8b", 1, 8))
    assert R.MODELS == {"llama2-7b": (32, 32, 128), "llama3-8b": (32, 8, 128)}
