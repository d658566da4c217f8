"""The host side of the block-scaled batched decode projection (sli_batch_gemm_mx8) and of sli_model_set_decode: symbols,
the planner and the refusals that need no device."""
import ctypes

import pytest

from simplellminference_amd import _lib

# the five batched launches of Llama-3-8B at batch 8: (rows, K, norm)
C4 = {"qkv": (6144, 4096, 1), "wo": (4096, 4096, 0), "gate_up": (28672, 4096, 1), "down": (4096, 14336, 0),
      "lm": (128256, 4096, 1)}


def _plan(rows, K, B, norm, tiled=1):
    p = _lib.BgemmMx8Plan()
    return p, _lib.load().sli_batch_gemm_mx8_workspace_bytes(rows, K, B, norm, tiled, ctypes.byref(p))


def test_symbols():
    lib = _lib.load()
    for name in ("sli_batch_gemm_mx8", "sli_batch_gemm_mx8_workspace_bytes", "sli_matmul_batch_mx8",
                 "sli_matmul_batch_mx8_workspace_bytes", "sli_model_set_decode", "sli_model_decode_path"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()


@pytest.mark.parametrize("rows,K,B", [(4096, 96, 8), (4096, 4096, 9), (4096, 4096, 0)])
def test_refused_shapes(rows, K, B):
    assert _plan(rows, K, B, 0)[1] == 0
    assert _lib.load().sli_matmul_batch_mx8_workspace_bytes(rows, K, B, 0) == 0


@pytest.mark.parametrize("name", sorted(C4))
def test_c4_plans(name):
    rows, K, norm = C4[name]
    p, nbytes = _plan(rows, K, 8, norm)
    ntiles = rows // 16
    assert p.wt * p.wk == 16 and p.tpw >= 1 and p.groups == -(-ntiles // p.tpw) and (p.splits == 1 or not norm)
    assert p.lds_bytes <= 160 * 1024 and nbytes >= ntiles * (K // 32) * (256 + 16)  # both images fit the workspace


def test_set_decode_arguments():
    lib = _lib.load()
    assert lib.sli_model_set_decode(None, 1) == 1 and b"null model" in lib.sli_last_error()  # SLI_ERR_ARG
    assert lib.sli_model_set_decode(None, 7) == 1 and b"unknown decode mode" in lib.sli_last_error()  # the mode is checked first
    assert lib.sli_model_decode_path(None) == 0
