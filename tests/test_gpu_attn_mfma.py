"""The MFMA decode attention (attn_mfma.h: one body, an fp16 and an FP8 E4M3 cache format) over every
(cache format, head_dim, query heads per kv head, ring depth) cell the default build can launch, against the oracle.

Two kv heads, so the kv-head index is not always 0. Contexts on a 256-CU part:
  T = 384:  hd 128 -> one tile per wave (ring depth 1), 3 splits of 128 keys; hd 64 -> the launch never splits below
            256 keys, so 2 tiles per wave (depth 2), 2 splits.
  T = 4224: more than 2048 x 2 keys per head under the 16-split cap -> 3 tiles per wave, so the depth-2 ring is
            refilled; 11 splits of 384 keys.
Positions T - 1 and T - 201: the second leaves the last live split with waves of unequal live-tile counts and a
masked tail inside a tile.

Bar: test_gpu_ops.py::test_mha's and test_gpu_kv8.py::test_mha_f8's, rtol 1e-5, atol 2e-6 against the oracle on the
cache's exact values, with their input construction.
"""
import functools

import numpy as np
import pytest

from tests.test_gpu_kv8 import _close, _mha_case, _t

pytestmark = pytest.mark.gpu

HKV, LAYER = 2, 1


@functools.lru_cache(maxsize=None)
def _mha_case_f16(T, hd, H, Hkv, pos):
    """test_mha's inputs: q and an fp16 cache of random normal values (as fp32, exactly representable)."""
    r = np.random.default_rng(T + pos)
    kv = Hkv * hd
    q = r.standard_normal(H * hd).astype(np.float32)
    kc = r.standard_normal((2, T, kv)).astype(np.float32).astype(np.float16).astype(np.float32)
    vc = r.standard_normal((2, T, kv)).astype(np.float32).astype(np.float16).astype(np.float32)
    return q, kc, vc


@pytest.mark.parametrize("back", [1, 201])
@pytest.mark.parametrize("T", [384, 4224])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("fmt", ["f16", "f8"])
def test_mha_mfma_grid(gpu, oracle, fmt, hd, G, T, back):
    torch = gpu
    from simplellminference_amd import ops
    H, pos = G * HKV, T - back
    if fmt == "f16":
        q, kf, vf = _mha_case_f16(T, hd, H, HKV, pos)
        got = ops.mha(_t(torch, q), _t(torch, kf).to(torch.float16), _t(torch, vf).to(torch.float16), LAYER, pos, T, hd,
                      H, HKV)
    else:
        q, kq, vq, kf, vf = _mha_case(T, hd, H, HKV, pos)
        got = ops.mha(_t(torch, q), _t(torch, kq), _t(torch, vq), LAYER, pos, T, hd, H, HKV, kv_dtype="f8")
    want = oracle.mha(q, kf, vf, LAYER, pos, T, hd, H, HKV)
    _close(got.cpu().numpy(), want, rtol=1e-5, atol=2e-6)
