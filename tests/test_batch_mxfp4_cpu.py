"""The host side of MXFP4 weights at batch > 1 (sli.h sli_batch_gemm_mxfp4, sli_matmul_batch_mxfp4,
sli_model_create_flags, sli_tp_group_create_flags): symbols, the workspace sizes, the refusals decided before the
device is touched, and the opt-in flag's argument checks. No test here makes a call that would pass the checks.
"""
import ctypes

import pytest

from simplellminference_amd import _lib, ops  # (ops imports torch ahead of libsli.so, as the GPU files do)
from tests.test_batch_stage_cpu import GATE_UP, LOGITS, PTR, QKV, STORE, _epi

ERR_ARG = 1
NEW = ("sli_batch_gemm_mxfp4", "sli_batch_gemm_mxfp4_workspace_bytes", "sli_matmul_batch_mxfp4",
       "sli_matmul_batch_mxfp4_workspace_bytes", "sli_model_create_flags", "sli_tp_group_create_flags")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exist(lib):
    assert set(NEW) <= set(_lib.exported_symbols())
    for name in NEW:
        assert hasattr(lib, name)
    assert callable(ops.matmul_batch_mxfp4) and _lib.CREATE_MX_BATCH == 1


def _plan(rows, K, B, norm, tiled=False, plan=None):
    return ops.batch_gemm_plan(rows, K, B, norm, _lib.DT_MXFP4, tiled, plan)


# ---------------------------------------------------------------- workspace bytes
@pytest.mark.parametrize("rows,K,plan", [(70, 544, (1, 1)), (512, 4096, None), (70, 7168, (2, 2)), (100, 256, None)])
def test_tiled_workspace_holds_both_images(rows, K, plan):
    norm = plan is None
    p0, plain = _plan(rows, K, 8, norm, False, plan)
    p1, tiled = _plan(rows, K, 8, norm, True, plan)
    images = ((rows + 15) // 16) * (K // 32) * (256 + 16)
    assert plain > 0 and p0 == p1
    assert plain + images <= tiled <= plain + images + 256
    # the plan is the fp16 / int8 entry's: the k-block stays the unit of everything
    assert p0 == ops.batch_gemm_plan(rows, K, 8, norm, _lib.DT_I8, False, plan)[0]


def test_workspace_bytes_are_zero_for_what_the_call_refuses(lib):
    assert _plan(70, 48, 8, False)[1] == 0          # K % 32
    assert _plan(70, 0, 8, False)[1] == 0
    assert _plan(70, 64, 0, False)[1] == 0          # B outside 1..8
    assert _plan(70, 64, 9, False)[1] == 0
    assert _plan(0, 64, 8, False)[1] == 0
    assert _plan(70, 544, 8, False, plan=(1, 2))[1] == 0    # a wave without a k-block of a split
    assert _plan(70, 1024, 8, True, plan=(1, 2))[1] == 0    # the fused norm runs on one split
    assert _plan(70, 4096, 8, True, plan=(31, 1))[1] == 0   # LDS
    assert _plan(70, 4096, 8, True, plan=(30, 1))[1] > 0
    assert _plan(70, 4128, 8, True)[1] == 0                 # staging registers
    assert _plan(70, 7168, 8, False, plan=(2, 2))[0]["step_width"] == 7
    ws = lib.sli_matmul_batch_mxfp4_workspace_bytes
    for tiled in (0, 1):
        assert ws(64, 48, 4, tiled) == 0 and ws(64, 128, 0, tiled) == 0 and ws(64, 128, 9, tiled) == 0
        assert ws(0, 128, 4, tiled) == 0 and ws(64, 0, 4, tiled) == 0


# ---------------------------------------------------------------- refusals without a device
def _refused(lib, role, why, K=544, B=8, plan=(1, 1), norm="role", x=PTR, data=PTR, scales=PTR, ws=PTR,
             ws_bytes=1 << 40, tiled=0, **epi):
    p = _lib.BgemmPlan(tpw=plan[0], splits=plan[1])
    e = _epi(role, **epi)
    norm_w = (None if role == STORE else PTR) if norm == "role" else norm
    rc = lib.sli_batch_gemm_mxfp4(x, norm_w, 1e-5, data, scales, tiled, K, B, ctypes.byref(e), ctypes.byref(p), ws,
                                  ws_bytes, None)
    msg = (lib.sli_last_error() or b"").decode()
    assert rc == ERR_ARG and why in msg and "sli_batch_gemm_mxfp4" in msg, (rc, msg)


@pytest.mark.parametrize("role", [QKV, GATE_UP, STORE, LOGITS])
def test_argument_checks_without_a_device(lib, role):
    _refused(lib, role, "null pointer", scales=None)
    _refused(lib, role, "null pointer", data=None)
    _refused(lib, role, "null pointer", x=None)
    _refused(lib, role, "null pointer", ws=None)
    _refused(lib, role, "16-byte alignment", scales=PTR + 8)
    _refused(lib, role, "16-byte alignment", data=PTR + 4)
    _refused(lib, role, "multiple of 32", K=48)
    _refused(lib, role, "batch must be in [1, 8]", B=9)
    _refused(lib, role, "LDS image too large", K=4096, plan=(31, 1))
    _refused(lib, role, "workspace too small", ws_bytes=16)
    _refused(lib, role, "workspace too small", tiled=1, ws_bytes=_plan(70, 544, 8, role != STORE, plan=(1, 1))[1])
    if role == STORE:
        _refused(lib, role, "no fused RMSNorm", norm=PTR)  # a norm with the store role
        _refused(lib, role, "every wave needs a k-block", K=544, plan=(1, 2))
    else:
        _refused(lib, role, "has the fused RMSNorm", norm=None)
        _refused(lib, role, "runs on one split", K=1024, plan=(1, 2))


def test_plain_rows_entry_refuses_without_a_device(lib):
    f = lib.sli_matmul_batch_mxfp4
    assert f(PTR, PTR, None, PTR, 64, 128, 4, 0, PTR, 1 << 30, None) == ERR_ARG  # null scales
    assert b"null pointer" in lib.sli_last_error()
    assert f(PTR, PTR, PTR, PTR, 64, 128, 4, 0, None, 1 << 30, None) == ERR_ARG
    assert f(PTR, PTR, PTR, PTR, 64, 48, 4, 0, PTR, 1 << 30, None) == 2          # SLI_ERR_SHAPE, as the int8 entry
    assert f(PTR, PTR, PTR, PTR, 64, 128, 9, 0, PTR, 1 << 30, None) == 2
    assert f(PTR + 4, PTR, PTR, PTR, 64, 128, 4, 0, PTR, 1 << 30, None) == ERR_ARG


def test_the_fp16_int8_entry_keeps_refusing_mxfp4(lib):
    p = _lib.BgemmPlan(tpw=1, splits=1)
    e = _epi(STORE)
    rc = lib.sli_batch_gemm(PTR, None, 1e-5, PTR, 3, None, 0, 544, 8, ctypes.byref(e), ctypes.byref(p), PTR, 1 << 40, None)
    assert rc == ERR_ARG and b"fp16 or int8 weights" in lib.sli_last_error()
    assert ops.batch_gemm_plan(70, 544, 8, False, _lib.DT_F32)[1] == 0
    q = _lib.BgemmPlan()
    assert lib.sli_batch_gemm_workspace_bytes(70, 544, 8, 0, 3, 0, ctypes.byref(q)) == 0


# ---------------------------------------------------------------- the creation flag
def _cfg(w_dtype, batch, **over):
    c = dict(vocab=256, dim=64, n_heads=1, n_kv_heads=1, head_dim=64, ffn=128, n_layers=1, max_len=16, eps=1e-5,
             theta=10000.0, w_dtype=w_dtype, kv_dtype=_lib.DT_F16, act_mode=0, tp_rank=0, tp_size=1, device=0, batch=batch)
    c.update(over)
    return _lib.ModelConfig(*c.values())


def test_create_flags_argument_checks(lib):
    h = ctypes.c_void_p()
    for flags in (2, 3, 0x80000000):  # an unknown bit, alone or beside the known one
        rc = lib.sli_model_create_flags(ctypes.byref(_cfg(_lib.DT_MXFP4, 2)), None, flags, ctypes.byref(h))
        assert rc == ERR_ARG and b"unknown flag bit" in lib.sli_last_error() and not h.value
        rc = lib.sli_tp_group_create_flags(ctypes.byref(_cfg(_lib.DT_MXFP4, 2)), 1, flags, ctypes.byref(h))
        assert rc == ERR_ARG and b"unknown flag bit" in lib.sli_last_error() and not h.value
    # the flag does nothing for fp32 weights: batch 2 is refused with the old message, with and without it
    for flags in (0, 1):
        rc = lib.sli_model_create_flags(ctypes.byref(_cfg(_lib.DT_F32, 2)), None, flags, ctypes.byref(h))
        assert rc == ERR_ARG and not h.value
        assert b"batch > 1 needs fp16 or int8 weights (MFMA projections)" in lib.sli_last_error()
    # without the flag MXFP4 at batch 2 is refused as before, through either entry
    rc = lib.sli_model_create_flags(ctypes.byref(_cfg(_lib.DT_MXFP4, 2)), None, 0, ctypes.byref(h))
    assert rc == ERR_ARG and b"batch > 1 needs fp16 or int8 weights (MFMA projections)" in lib.sli_last_error()
    rc = lib.sli_model_create(ctypes.byref(_cfg(_lib.DT_MXFP4, 2)), None, ctypes.byref(h))
    assert rc == ERR_ARG and b"batch > 1 needs fp16 or int8 weights (MFMA projections)" in lib.sli_last_error()
    # with it the remaining batched limits still hold (decided before the device is touched)
    rc = lib.sli_model_create_flags(ctypes.byref(_cfg(_lib.DT_MXFP4, 9)), None, 1, ctypes.byref(h))
    assert rc == 2 and b"batch must be at most 8" in lib.sli_last_error()
