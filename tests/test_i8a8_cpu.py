"""The host side of the integer-MFMA prefill (sli_prefill_gemm_i8a8 and its quantisers): symbols, and every refusal that
is decided before the device is touched."""
import ctypes

import pytest

from simplellminference_amd import _lib

A = 0x10000  # a 16-byte aligned non-null address; no refusal below reads through it


def test_symbols():
    lib = _lib.load()
    for name in ("sli_prefill_norm_quant_i8", "sli_prefill_quant_i8", "sli_prefill_gemm_i8a8"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()


def _gemm(w=A, rs=A, ac=A, a_s=A, N=16, K=128, M=32, p0=0, nv=32, state=A, role=2, y=A):
    e = _lib.PgemmEpilogue(role=role, y=y, ld=N)
    lib = _lib.load()
    rc = lib.sli_prefill_gemm_i8a8(w, rs, ac, a_s, N, K, M, p0, nv, ctypes.byref(e), state, None, None)
    return rc, lib.sli_last_error()


@pytest.mark.parametrize("over,code,word", [
    (dict(K=192), 2, b"multiple of 128"), (dict(K=64), 2, b"multiple of 128"), (dict(K=131072 + 128), 2, b"131072"),
    (dict(w=None), 1, b"null"), (dict(ac=None), 1, b"null"), (dict(a_s=None), 1, b"null"), (dict(state=None), 1, b"null"),
    (dict(y=None), 1, b"null y"), (dict(w=A + 8), 1, b"alignment"), (dict(ac=A + 4), 1, b"alignment"),
    (dict(rs=A + 4), 1, b"alignment"), (dict(a_s=A + 2), 1, b"alignment"), (dict(state=A + 4), 1, b"alignment"),
    (dict(M=48), 1, b"M must be"), (dict(N=24), 1, b"multiple of 16"), (dict(nv=33), 1, b"nv"), (dict(role=4), 1, b"role"),
])
def test_gemm_refusals(over, code, word):
    rc, why = _gemm(**over)
    assert rc == code and word in why, (rc, why)


@pytest.mark.parametrize("fn,args,word", [
    ("sli_prefill_norm_quant_i8", (None, None, A, A, 4, 128, 0.0, None), b"null"),
    ("sli_prefill_norm_quant_i8", (A, A, A, A, 4, 16384, 0.0, None), b"8192"),
    ("sli_prefill_norm_quant_i8", (A, None, A, A, 4, 130, 0.0, None), b"multiple of 4"),
    ("sli_prefill_norm_quant_i8", (A + 4, None, A, A, 4, 128, 0.0, None), b"alignment"),
    ("sli_prefill_quant_i8", (A, None, A, A, 4, 128, None), b"null"),
    ("sli_prefill_quant_i8", (A, A, A, A, 0, 128, None), b"M must be"),
    ("sli_prefill_quant_i8", (A, A, A + 8, A, 4, 128, None), b"alignment"),
])
def test_quant_refusals(fn, args, word):
    lib = _lib.load()
    assert getattr(lib, fn)(*args) == 1 and word in lib.sli_last_error()  # SLI_ERR_ARG


def test_mode_6_is_unknown():
    lib = _lib.load()
    assert lib.sli_model_set_prefill(None, 6) == 1 and b"mode must be" in lib.sli_last_error()
    assert lib.sli_model_set_prefill(None, 5) == 1 and b"null" in lib.sli_last_error()  # 5 is a mode: the model is missing
