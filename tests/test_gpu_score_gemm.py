"""The logits epilogue (role 3) of the prefill GEMM (csrc/prefill.h PgEpiLogits), one launch at a time through
ops.prefill_gemm_logits, against the float64 reference tests/prefill_ref.py on the identical rounded operands.

Bar: the role-2 bound of tests/test_gpu_prefill_kernels.py, bar (c): the sum within dY = 4 eps32 sqrt(K) (|W| @ (|hi| +
|lo|)) of the float64 sum, times the row scale, plus the scale multiply's own rounding: dY sc + eps32 |Y sc|. N need not
be a multiple of 16; y is pre-filled with a sentinel that columns N .. ld - 1 must keep; for N % 16 == 0 the result is
bit-equal to role 2 with a null residual.
"""
import numpy as np
import pytest

from tests import mxfp4_prefill_ref as G
from tests import mxfp4_ref as mx
from tests import prefill_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 1024, 32), (512, 256, 64), (1000, 1024, 256)]  # (N, K, M)
SENT32 = 0x7FC5A5A5  # a NaN bit pattern no kernel result equals


def _t(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _weights(torch, oracle, w, N, K, seed):
    """N(0, 1 / K) weights: (device operands as keyword arguments, the float64-exact matrix, the row scales)."""
    from simplellminference_amd import ops
    w32 = (np.random.default_rng(seed).standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    if w == "f16":
        W = w32.astype(np.float16)
        return dict(w=_t(torch, W)), W, None
    if w == "i8":
        q, s = np.empty((N, K), np.int8), np.empty(N, np.float32)
        for i in range(N):
            q[i], s[i] = oracle.quant_row_i8(w32[i])
        return dict(w=_t(torch, q), row_scale=_t(torch, s)), q, s
    data, scales = ops.quant_mxfp4(_t(torch, w32))
    return dict(w=data, scales=scales), G.weights64(mx.unpack(data.cpu().numpy()), scales.cpu().numpy()), None


def _acts(torch, M, K, seed):
    from simplellminference_amd import ops
    x = np.random.default_rng(seed).standard_normal((M, K)).astype(np.float32)
    return ops.prefill_norm_split(_t(torch, x), None, 1e-5)


@pytest.mark.parametrize("N,K,M", SHAPES)
@pytest.mark.parametrize("w", ["f16", "i8", "mxfp4"])
def test_logits_role(gpu, oracle, w, N, K, M):
    torch = gpu
    from simplellminference_amd import ops
    kw, W, scale = _weights(torch, oracle, w, N, K, 7 * M + N)
    hi, lo = _acts(torch, M, K, 3 * M + N)
    ld = (N + 3) // 4 * 4 + 8
    y = torch.full((M, ld), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    ops.prefill_gemm_logits(kw["w"], hi, lo, y, row_scale=kw.get("row_scale"), scales=kw.get("scales"))
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert (got[:, N:].view(np.uint32) == SENT32).all(), "columns N .. ld - 1 were written"
    assert not (got[:, :N].view(np.uint32) == SENT32).any(), "a column below N was not written"
    hi_h, lo_h = hi.cpu().numpy(), lo.cpu().numpy()
    Y = R.gemm_sums(W, hi_h, lo_h)
    dY = 4 * R.EPS32 * np.sqrt(K) * R.gemm_abs(W, hi_h, lo_h)
    sc = 1.0 if scale is None else scale.astype(np.float64)
    ref = R.epi_resid(Y, scale, None)
    tol = dY * sc + R.EPS32 * np.abs(Y * sc)
    err = np.abs(got[:, :N].astype(np.float64) - ref)
    print(f"{w} N {N} K {K} M {M}: max err / tol {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), float((err / tol).max())
    if N % 16 == 0:
        y2 = torch.full((M, ld), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
        ops.prefill_gemm_resid(kw["w"], hi, lo, y2, resid=None, row_scale=kw.get("row_scale"), scales=kw.get("scales"))
        torch.cuda.synchronize()
        assert np.array_equal(y2.cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_the_entry_refuses_what_the_role_cannot_take(gpu):
    torch = gpu
    from simplellminference_amd import ops
    from simplellminference_amd._lib import SliError
    f16 = lambda *s: torch.zeros(*s, dtype=torch.float16, device="cuda")
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    for args in ((f16(8, 64), f16(32, 64), f16(32, 64), f32(32, 8)),       # N < 16
                 (f16(24, 64), f16(32, 64), f16(32, 64), f32(32, 20)),     # ld < N
                 (f16(24, 64), f16(32, 64), f16(32, 64), f32(32, 26))):    # ld % 4
        with pytest.raises(SliError) as e:
            ops.prefill_gemm_logits(*args)
        assert e.value.code == 1
    y = f32(32, 24)
    ops.prefill_gemm_logits(f16(24, 64), f16(32, 64), f16(32, 64), y)      # and a good N that is no multiple of 16
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0
