"""sli_decode_gemv (include/sli.h "decode stages, for tests and labs") without a GPU: the symbols, every refusal with
its message (no call here would pass the checks, so nothing reaches a device), the schedule facts the comments of gemv.h
state, reproduced by sli_decode_gemv_plan at 256 compute units, and the coverage condition of the GPU file's cells."""
import ctypes

import pytest

from simplellminference_amd import _lib, ops
from tests import gemv_ref as G

DT = {"f32": _lib.DT_F32, "f16": _lib.DT_F16, "i8": _lib.DT_I8, "mxfp4": _lib.DT_MXFP4}
A = 0x10000  # a 16-byte aligned address that is never dereferenced: every call below is refused on the host


def test_symbols():
    lib = _lib.load()
    for name in ("sli_decode_gemv", "sli_decode_gemv_mxfp4", "sli_decode_gemv_plan"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()


def _call(e, cols=4096, x=A, norm_w=None, w=A, w_dtype=_lib.DT_F16, rs=None, cus=256, mx=False):
    p = _lib.GemvPlan(cus=cus)
    lib = _lib.load()
    if mx:
        rc = lib.sli_decode_gemv_mxfp4(x, norm_w, 1e-5, w, A, cols, ctypes.byref(e), ctypes.byref(p), None)
    else:
        rc = lib.sli_decode_gemv(x, norm_w, 1e-5, w, w_dtype, rs, cols, ctypes.byref(e), ctypes.byref(p), None)
    return rc, (lib.sli_last_error() or b"").decode()


def _qkv(**kw):
    f = dict(role=G.QKV, q=A, kc=A, vc=A, pos=A, sin_t=A, cos_t=A, hq=4, hkv=2, hd=64, T=40, kv_dtype=_lib.DT_F16)
    f.update(kw)
    return _lib.GemvEpilogue(**f)


def _wo(**kw):
    f = dict(role=G.WO, y=A, nrows=64)
    f.update(kw)
    return _lib.GemvEpilogue(**f)


def _merged(**kw):
    f = dict(part=A, pos=A, hq=32, hd=128, max_splits=8, ppwg=4)
    f.update(kw)
    return _wo(**f)


REFUSALS = [
    ("misaligned x", lambda: _call(_wo(), x=A + 4), "16-byte alignment"),
    ("misaligned weights", lambda: _call(_wo(), w=A + 8), "16-byte alignment"),
    ("misaligned row scale", lambda: _call(_wo(), rs=A + 4), "16-byte alignment"),
    ("misaligned output", lambda: _call(_wo(y=A + 4)), "16-byte alignment"),
    ("misaligned partials", lambda: _call(_merged(part=A + 8), x=None), "16-byte alignment"),
    ("misaligned position", lambda: _call(_qkv(pos=A + 4), norm_w=A), "16-byte alignment"),
    ("misaligned keys", lambda: _call(_lib.GemvEpilogue(role=G.LOGITS, logits=A, keys=A + 8, nrows=9, key_ld=256), norm_w=A),
     "16-byte alignment"),
    ("fp32 columns", lambda: _call(_wo(), cols=4098, w_dtype=_lib.DT_F32), "multiple of the weight type's vector width"),
    ("fp16 columns", lambda: _call(_wo(), cols=4100), "multiple of the weight type's vector width"),
    ("int8 columns", lambda: _call(_wo(), cols=4104, w_dtype=_lib.DT_I8), "multiple of the weight type's vector width"),
    ("mxfp4 columns", lambda: _call(_wo(), cols=4112, mx=True), "multiple of the weight type's vector width"),
    ("too many columns", lambda: _call(_wo(), cols=16384), "exceeds the staged input"),
    ("mxfp4 through the plain entry", lambda: _call(_wo(), w_dtype=_lib.DT_MXFP4), "fp32, fp16 or int8 weights"),
    ("bad role", lambda: _call(_lib.GemvEpilogue(role=7)), "role must be"),
    ("cus above the device's", lambda: _call(_wo(), cus=100000), "cus exceeds"),
    ("negative cus", lambda: _call(_wo(), cus=-1), "cus must be"),
    ("qkv without norm", lambda: _call(_qkv()), "q/k/v launch has the fused RMSNorm"),
    ("qkv head_dim", lambda: _call(_qkv(hd=96), norm_w=A), "head_dim must be 64 or 128"),
    ("qkv hq % hkv", lambda: _call(_qkv(hq=3), norm_w=A), "hq must be a multiple of hkv"),
    ("qkv kv dtype", lambda: _call(_qkv(kv_dtype=_lib.DT_I8), norm_w=A), "bad kv dtype"),
    ("qkv fp32 weights with an FP8 cache", lambda: _call(_qkv(kv_dtype=_lib.DT_F8E4M3), norm_w=A, w_dtype=_lib.DT_F32),
     "no fp32 weights with an FP8 cache"),
    ("qkv with partials", lambda: _call(_qkv(np=2, parts=A), norm_w=A), "stages a plain input"),
    ("qkv null cache", lambda: _call(_qkv(kc=None), norm_w=A), "null q/k/v operand"),
    ("gate/up without norm", lambda: _call(_lib.GemvEpilogue(role=G.GATE_UP, act=A, inter=64)), "gate/up launch has the fused RMSNorm"),
    ("gate/up np", lambda: _call(_lib.GemvEpilogue(role=G.GATE_UP, act=A, inter=64, np=3, parts=A), norm_w=A), "np must be 0, 2 or 4"),
    ("gate/up partials too wide", lambda: _call(_lib.GemvEpilogue(role=G.GATE_UP, act=A, inter=64, np=2, parts=A), norm_w=A, cols=4104),
     "cols <= 4096"),
    ("gate/up act_mode", lambda: _call(_lib.GemvEpilogue(role=G.GATE_UP, act=A, inter=64, act_mode=2), norm_w=A), "act_mode"),
    ("gate/up null partials", lambda: _call(_lib.GemvEpilogue(role=G.GATE_UP, act=A, inter=64, np=2), norm_w=A), "null partials"),
    ("wo with norm", lambda: _call(_wo(), norm_w=A), "wo launch has no fused RMSNorm"),
    ("wo with np", lambda: _call(_wo(np=2, parts=A)), "takes no partials"),
    ("wo null input", lambda: _call(_wo(), x=None), "null input"),
    ("merged head_dim", lambda: _call(_merged(hd=96), x=None), "head_dim must be 64 or 128"),
    ("merged cols != hq hd", lambda: _call(_merged(hq=31), x=None), "cols must be hq * hd"),
    ("merged splits", lambda: _call(_merged(max_splits=0), x=None), "max_splits and ppwg"),
    ("K-split without partials", lambda: _call(_wo(ks=2, kpart=A)), "merges its input"),
    ("K-split ks", lambda: _call(_merged(ks=3, kpart=A), x=None), "ks must be 1, 2 or 4"),
    ("K-split hq % ks", lambda: _call(_wo(part=A, pos=A, hq=6, hd=128, max_splits=8, ppwg=4, ks=4, kpart=A), cols=768, x=None),
     "hq must be a multiple of ks"),
    ("K-split no grid", lambda: _call(_merged(ks=4, kpart=A), x=None, cus=3), "no grid keeps every workgroup"),
    ("K-split null output", lambda: _call(_merged(ks=2), x=None), "null output"),
    ("down with norm", lambda: _call(_lib.GemvEpilogue(role=G.DOWN, y=A, nrows=64), norm_w=A), "down launch has no fused RMSNorm"),
    ("down summed residual without x", lambda: _call(_lib.GemvEpilogue(role=G.DOWN, y=A, nrows=64, np=2, parts=A)),
     "needs x (resid)"),
    ("logits without norm", lambda: _call(_lib.GemvEpilogue(role=G.LOGITS, logits=A, keys=A, nrows=9, key_ld=256)),
     "LM head launch has the fused RMSNorm"),
    ("logits key_ld", lambda: _call(_lib.GemvEpilogue(role=G.LOGITS, logits=A, keys=A, nrows=99, key_ld=1), norm_w=A, cus=4),
     "one key per workgroup"),
    ("logits vocab_off", lambda: _call(_lib.GemvEpilogue(role=G.LOGITS, logits=A, keys=A, nrows=9, key_ld=9, vocab_off=-1), norm_w=A),
     "vocab_off"),
    ("LDS", lambda: _call(_wo(nrows=100000), cols=16320, cus=1), "64 KiB of LDS"),
]


@pytest.mark.parametrize("what,fn,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, fn, msg):
    rc, err = fn()
    assert rc == 1, (what, rc, err)  # SLI_ERR_ARG
    assert msg in err, (what, err)


def _plan(role, wt, cols, cus=256, **shape):
    return ops.decode_gemv_plan(role, DT[wt], cols, cus=cus, **shape)


def test_schedule_facts_at_256_cus():
    """What the comments of gemv.h and engine.hip state about Llama-2-7B on 256 compute units."""
    gu = _plan(G.GATE_UP, "f16", 4096, inter=11008)
    assert (gu["grid"], gu["csplit"], gu["u"], gu["cw"]) == (230, 1, 4, 16)  # "gate/up: 230 workgroups", unsplit
    items = [c for wg in G.wave_items(gu) for c in wg]
    assert max(items) == 3 and 2.9 < sum(items) / len(items) < 3.0
    qkv = _plan(G.QKV, "i8", 4096, hq=32, hkv=32, hd=128, T=2048, kv_dtype=1)
    assert (qkv["grid"], qkv["units"], qkv["cw"], qkv["u"]) == (256, 6144, 12, 2)  # 24 units per workgroup: 12 waves of 2
    assert _plan(G.QKV, "f16", 4096, hq=32, hkv=32, hd=128, T=2048, kv_dtype=1)["cw"] == 16  # int8 weights only
    tp8 = _plan(G.QKV, "f16", 4096, hq=4, hkv=4, hd=128, T=2048, kv_dtype=1)
    assert (tp8["units"], tp8["csplit"]) == (768, 8)  # "TP-8 q/k/v has 768 two-row units for 4096 waves"
    lm = _plan(G.LOGITS, "f16", 4096, nrows=32000, key_ld=256)
    assert (lm["grid"], lm["units"]) == (256, 16000)  # the LM head keeps the full grid (2.4 % tail)
    down = _plan(G.DOWN, "i8", 11008, nrows=4096)
    assert (down["u"], down["chunks_per_row"], down["masked_tail"]) == (4, 3, 1)  # "int8 down at 7B, 3 chunks per row"
    wo = _plan(G.WO, "f16", 4096, nrows=4096, hq=32, hd=128, max_splits=8, ppwg=256, ks=2)
    assert (wo["grid"], wo["units"], wo["nb"], wo["ns"], wo["u"]) == (256, 8192, 4, 8, 2)
    assert _plan(G.WO, "f16", 4096, nrows=4096, merged=True, hq=32, hd=128, max_splits=16, ppwg=256)["ns"] == 16
    assert gu["lds_bytes"] == 4 * (64 + 4096) + 4 * 2 * (11008 // 230 + 2)


def _cell_classes(wt):
    out = {}
    for cell in G.CELLS:
        if G.cell_takes(cell, wt):
            role, cols, cus, shape = cell
            p = _plan(role, wt, cols, cus=cus, **dict(shape))
            assert p["lds_bytes"] <= 64 * 1024 and p["grid"] <= cus
            out[G.cell_id(cell)] = (G.schedule_class(role, p), p)
    return out


@pytest.mark.parametrize("wt", G.WTS)
def test_cells_cover_production(wt):
    """The schedule class of every GEMV launch of Llama-2-7B at TP 1, 4 and 8 and of Llama-3-8B is the class of a cell
    the GPU file runs with this weight type."""
    have = {c for c, _ in _cell_classes(wt).values()}
    missing = []
    for model, tp in G.PRODUCTION:
        for role, cols, shape in G.production_launches(model, tp):
            c = G.schedule_class(role, _plan(role, wt, cols, **dict(shape)))
            if c not in have:
                missing.append((model, tp, G.ROLE_NAMES[role], cols, shape, c))
    assert not missing, missing


@pytest.mark.parametrize("wt", G.WTS)
def test_cells_take_the_listed_branches(wt):
    cl = _cell_classes(wt)
    plans = [p for _, p in cl.values()]
    classes = [c for c, _ in cl.values()]
    assert any(p["chunks_per_row"] == 1 and p["masked_tail"] for p in plans)      # one chunk, masked
    assert any(p["chunks_per_row"] > 1 and not p["masked_tail"] for p in plans)   # chunks, full tail
    assert any(p["chunks_per_row"] > 1 and p["masked_tail"] for p in plans)       # chunks, masked tail
    assert any(c[5] == 3 and c[6] for c in classes)                                # >= 3 items on a wave, unequal waves
    assert any(c[7] for c in classes)                                              # waves with no item
    assert {2, 4} <= {p["csplit"] for p in plans}
    assert any(p["csplit"] > 1 and (p["csplit"] - 1) * p["chunks_per_part"] >= p["chunks_per_row"] for p in plans)
    assert any(p["units"] > 1024 and p["grid"] == 1 for p in plans)               # the non-prefetched epilogue path
    assert {8, 16} <= {p["ns"] for p in plans}
    if wt == "i8":
        assert any(p["cw"] == 12 for p in plans)
    if wt in ("f16", "f32"):
        assert 8 in {p["csplit"] for p in plans}
