"""The host side of the kernel-level entry for one batched decode projection (sli.h "batched decode stages, for tests
and labs": sli_batch_gemm, sli_batch_gemm_workspace_bytes): symbols, the workspace sizes, every refusal of a forced
plan or an operand (each SLI_ERR_ARG with its own message, decided before the device is touched: no test here makes
a call that would pass the checks), and the coverage condition: every plan class the engine's planner picks for the
batched launches of the production shapes at batch 8 is among the classes test_gpu_batch_kernels.py forces.
"""
import ctypes

import pytest

from simplellminference_amd import _lib, ops  # (ops imports torch ahead of libsli.so, as the GPU files do)
from tests import bgemm_ref as R

ERR_ARG = 1
QKV, GATE_UP, STORE, LOGITS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exist(lib):
    for name in ("sli_batch_gemm", "sli_batch_gemm_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    for name in ("batch_gemm_qkv", "batch_gemm_gate_up", "batch_gemm_store", "batch_gemm_logits", "batch_gemm_plan"):
        assert callable(getattr(ops, name))


def _plan(rows, K, B, norm, w_dtype=1, tiled=False, plan=None):
    return ops.batch_gemm_plan(rows, K, B, norm, w_dtype, tiled, plan)


# ---------------------------------------------------------------- refusals
_HOST = (ctypes.c_char * 65536)()
PTR = (ctypes.addressof(_HOST) + 255) & ~255  # host memory, 256-byte aligned: it passes the pointer checks only


def _epi(role, **over):
    base = {QKV: dict(q=PTR, kc=PTR, vc=PTR, kv_dtype=1, pos=PTR, sin_t=PTR, cos_t=PTR, hq=4, hkv=2, hd=64, T=40),
            GATE_UP: dict(act=PTR, inter=40, act_mode=1),
            STORE: dict(y=PTR, resid=PTR, scale=1.0, nrows=70, ld=96),
            LOGITS: dict(logits=PTR, keys_out=PTR, nrows=70, ld=96, vocab_off=1000, key_ld=8)}[role]
    base.update(over)
    return _lib.BgemmEpilogue(role=role, **base)


def _refused(lib, role, why, K=544, B=8, plan=(1, 1), w_dtype=1, norm="role", x=PTR, w=PTR, rs=None, ws=PTR,
             ws_bytes=1 << 40, tiled=0, **epi):
    """One sli_batch_gemm call that must be SLI_ERR_ARG with `why` in its message."""
    p = _lib.BgemmPlan(tpw=plan[0], splits=plan[1])
    e = _epi(role, **epi)
    norm_w = (None if role == STORE else PTR) if norm == "role" else norm
    rc = lib.sli_batch_gemm(x, norm_w, 1e-5, w, w_dtype, rs, tiled, K, B, ctypes.byref(e), ctypes.byref(p), ws,
                            ws_bytes, None)
    msg = (lib.sli_last_error() or b"").decode()
    assert rc == ERR_ARG and why in msg, (rc, msg)


@pytest.mark.parametrize("role", [QKV, GATE_UP, STORE, LOGITS])
def test_forced_plans_the_kernel_cannot_run_are_refused(lib, role):
    norm = role != STORE
    _refused(lib, role, "tpw and splits must be >= 1", plan=(-1, 1))
    _refused(lib, role, "tpw and splits must be >= 1", plan=(1, 0))
    _refused(lib, role, "tpw and splits must be >= 1", plan=(2, -3))
    _refused(lib, role, "LDS image too large", K=4096, plan=(31, 1))  # 1 + 128 + 16 + 15.5 KiB > 160 KiB
    _refused(lib, role, "LDS image too large", plan=(1 << 20, 1))
    _refused(lib, role, "multiple of 32", K=48)
    _refused(lib, role, "multiple of 32", K=0)
    _refused(lib, role, "batch must be in [1, 8]", B=0)
    _refused(lib, role, "batch must be in [1, 8]", B=9)
    if norm:
        _refused(lib, role, "runs on one split", K=1024, plan=(1, 2))
        _refused(lib, role, "exceeds the staging registers", K=4128)
        _refused(lib, role, "no plan fits", K=4128, plan=(0, 0))  # the automatic plan has none either
        _refused(lib, role, "has the fused RMSNorm", norm=None)
    else:
        _refused(lib, role, "every wave needs a k-block", K=992, plan=(1, 2))  # 31 blocks over 2 splits: 15 < 16 waves
        _refused(lib, role, "every wave needs a k-block", K=544, plan=(1, 2))
        _refused(lib, role, "exceeds the staging registers", K=4128)
        _refused(lib, role, "exceeds the staging registers", K=8256, plan=(1, 2))  # ceil(258 / 2) * 32 = 4128
        _refused(lib, role, "no fused RMSNorm", norm=PTR)


def test_operands_the_kernel_cannot_take_are_refused(lib):
    _refused(lib, QKV, "head_dim must be 64 or 128", hd=32)
    _refused(lib, QKV, "head_dim must be 64 or 128", hd=96)
    _refused(lib, QKV, "multiple of hkv", hq=3, hkv=2)
    _refused(lib, QKV, "multiple of hkv", hkv=0)
    _refused(lib, QKV, "bad kv dtype", kv_dtype=2)
    _refused(lib, QKV, "T must be positive", T=0)
    _refused(lib, QKV, "null q/k/v operand", pos=None)
    _refused(lib, GATE_UP, "multiple of 8", inter=44)
    _refused(lib, GATE_UP, "multiple of 8", inter=0)
    _refused(lib, GATE_UP, "act_mode", act_mode=2)
    _refused(lib, STORE, "ld must be >= nrows", ld=64)
    _refused(lib, STORE, "ld must be >= nrows", nrows=0)
    _refused(lib, LOGITS, "ld must be >= nrows", ld=69)
    _refused(lib, LOGITS, "vocab_off", vocab_off=-1)
    _refused(lib, LOGITS, "one key per workgroup group", key_ld=4)  # 5 tiles, tpw 1: 5 groups
    _refused(lib, LOGITS, "one key per workgroup group", key_ld=1, plan=(3, 1))  # 2 groups
    for role in (QKV, GATE_UP, STORE, LOGITS):
        _refused(lib, role, "fp16 or int8 weights", w_dtype=0)
        _refused(lib, role, "fp16 or int8 weights", w_dtype=3)
        _refused(lib, role, "null pointer", x=None)
        _refused(lib, role, "null pointer", ws=None)
        _refused(lib, role, "workspace too small", ws_bytes=16)
        _refused(lib, role, "workspace too small", tiled=1, ws_bytes=_plan(70, 544, 8, role != STORE, plan=(1, 1))[1])
        for name in ("x", "w", "rs", "ws"):
            _refused(lib, role, "16-byte alignment", **{name: PTR + 8})
        if role != STORE:
            _refused(lib, role, "16-byte alignment", norm=PTR + 4)
    for role, fields in ((QKV, ("q", "kc", "vc", "pos", "sin_t", "cos_t")), (GATE_UP, ("act",)), (STORE, ("y", "resid")),
                         (LOGITS, ("logits", "keys_out"))):
        for f in fields:
            _refused(lib, role, "16-byte alignment", **{f: PTR + 8})
    p = _lib.BgemmPlan(tpw=1, splits=1)
    e = _lib.BgemmEpilogue(role=4)
    assert lib.sli_batch_gemm(PTR, None, 0.0, PTR, 1, None, 0, 64, 1, ctypes.byref(e), ctypes.byref(p), PTR, 1 << 30,
                              None) == ERR_ARG
    assert b"role must be" in lib.sli_last_error()


def test_plan_function_refuses_what_the_call_refuses():
    assert _plan(70, 544, 8, False, plan=(1, 2))[1] == 0
    assert _plan(70, 1024, 8, True, plan=(1, 2))[1] == 0
    assert _plan(70, 4096, 8, True, plan=(31, 1))[1] == 0
    assert _plan(70, 4096, 8, True, plan=(30, 1))[1] > 0
    assert _plan(70, 48, 8, False)[1] == 0
    assert _plan(70, 64, 9, False)[1] == 0
    assert _plan(0, 64, 8, False)[1] == 0
    assert _plan(70, 64, 8, False, w_dtype=0)[1] == 0
    assert _plan(70, 4128, 8, True)[1] == 0


# ---------------------------------------------------------------- plans and workspace
def test_forced_plan_is_reported_as_it_runs():
    p, n = _plan(70, 7168, 8, False, plan=(2, 2))
    assert (p["tpw"], p["splits"], p["groups"], p["step_width"]) == (2, 2, 3, 7)
    assert p["lds_bytes"] == 1024 + 112 * 1024 + 16384 + 2 * 512
    assert p["counter_off"] == 5 * 2 * 128 * 4 and n >= p["counter_off"] + 4 * p["groups"]
    assert _plan(70, 3584, 8, False, plan=(1, 1))[0]["step_width"] == 2   # one tile per workgroup: the finer pipeline
    assert _plan(70, 3584, 8, False, plan=(2, 1))[0]["step_width"] == 7   # 7 blocks per wave in one step
    assert _plan(70, 3072, 8, False, plan=(2, 1))[0]["step_width"] == 7   # 6: one clamped duplicate
    assert _plan(70, 2560, 8, False, plan=(2, 1))[0]["step_width"] == 4
    assert _plan(70, 3584, 8, True, plan=(2, 1))[0]["step_width"] == 4    # no width 7 with a norm
    assert _plan(70, 64, 8, True, plan=(17, 1))[0]["groups"] == 1
    assert _plan(550, 64, 8, True, plan=(17, 1))[0]["groups"] == 3
    p, _ = _plan(70, 544, 8, True, plan=(3, 1))
    assert p["counter_off"] == 0  # one split: no partials


@pytest.mark.parametrize("w_dtype,esize", [(1, 2), (2, 1)])
@pytest.mark.parametrize("rows,K,plan", [(70, 544, (1, 1)), (512, 4096, None), (70, 7168, (2, 2))])
def test_tiled_workspace_grows_by_the_image(w_dtype, esize, rows, K, plan):
    norm = plan is None
    _, plain = _plan(rows, K, 8, norm, w_dtype, False, plan)
    _, tiled = _plan(rows, K, 8, norm, w_dtype, True, plan)
    image = ((rows + 15) // 16) * (K // 32) * 512 * esize
    assert image >= rows * K * esize and plain > 0
    assert plain + image <= tiled <= plain + image + 256


# ---------------------------------------------------------------- coverage
def _tested_classes():
    out = set()
    for role in ("qkv", "gate_up", "store", "logits"):
        for shape, K, tpw, s in R.cells(role):
            p, n = _plan(R.rows_of(role, shape), K, 8, role != "store", plan=(tpw, s))
            assert n > 0, (role, shape, K, tpw, s)
            out.add(R.plan_class(p, K, role != "store"))
    return out


def _launches(cfg, tp):
    """(name, rows, K, norm) of the five batched launches per layer and step of a config's rank under TP `tp`."""
    hd = cfg.head_dim
    hq, hkv = cfg.num_attention_heads // tp, cfg.num_key_value_heads // tp
    D, I = cfg.hidden_size, cfg.intermediate_size // tp
    return [("qkv", (hq + 2 * hkv) * hd, D, True), ("wo", D, hq * hd, False), ("gate/up", 2 * I, D, True),
            ("down", D, I, False), ("lm head", cfg.vocab_size // tp, D, True)]


@pytest.mark.parametrize("name,tp", [("llama3-8b", 1), ("llama2-7b", 1), ("llama3-8b", 8), ("small-h128-gqa", 1),
                                     ("tiny-gqa", 1)])
def test_every_production_plan_class_is_forced_on_the_gpu(name, tp):
    """The planner's answer (256 CUs without a device, the MI355X's count) for each batched launch at batch 8: its
    class must be one the GPU file forces. A planner change that moves a production launch into an untested class
    fails here, on the CPU."""
    from simplellminference_amd.model import preset
    tested = _tested_classes()
    missing = []
    for what, rows, K, norm in _launches(preset(name), tp):
        p, n = _plan(rows, K, 8, norm)
        assert n > 0
        c = R.plan_class(p, K, norm)
        print(f"{name} TP-{tp} {what}: {rows} x {K} -> tpw {p['tpw']} splits {p['splits']} width {p['step_width']}, class {c}")
        if c not in tested:
            missing.append((what, c))
    assert not missing, missing

