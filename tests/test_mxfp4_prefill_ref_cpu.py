"""tests/mxfp4_prefill_ref.py against the conditions it states, without a GPU: every grid case the GPU tests of the
MXFP4 prefill GEMM draw stays below 2^24 product units, fp32 sums of such operands do not depend on the order, and
libsli.so carries the new entry points."""
import ctypes

import numpy as np

from tests import mxfp4_prefill_ref as G
from tests import mxfp4_ref as mx
from tests import prefill_ref as R


def test_every_grid_case_stays_below_2_24_units():
    cases = G.all_grid_cases()
    assert len(cases) == 3 * 4 * 6 + 4 + 1 + 3 + 4  # 12 cells x 6 depths (+ the hd 128 shape), range, bounds
    worst = 0.0
    for N, K, M, seed, centres in cases:
        codes, scales, hi, lo = G.grid_inputs(N, K, M, seed, centres=centres)
        w = G.window_for(K)
        assert K * 12 * 2 ** (w - 1) * 16 < 2 ** 24, (K, w)  # the worst case the module docstring derives
        e = scales.astype(int) - 127
        assert (e.max(axis=1) - e.min(axis=1) < w).all()
        assert len(np.unique(codes)) == 16
        u = G.grid_units(codes, scales, hi, lo)
        worst = max(worst, u)
        assert u < 2 ** 24, (N, K, M, seed, u)
    print(f"largest sum of magnitudes: {worst:.0f} units = 2^{np.log2(worst):.2f}")
    e = G.grid_inputs(G.N_RESID, 704, 64, 77, centres=G.range_centres(G.N_RESID))[1].astype(int) - 127
    assert e.min() <= -100 and e.max() >= 100 and ((e < -24) | (e > 15)).mean() > 0.5  # outside fp16's exponents


def _fp32_sums(W32, h32, order):
    acc = np.zeros((h32.shape[0], W32.shape[0]), np.float32)
    for k in order:
        acc += np.outer(h32[:, k], W32[:, k]).astype(np.float32)  # the product, rounded to fp32, then the add
    return acc


def test_fp32_sums_in_two_orders_equal_float64():
    """Forward and a shuffled order in fp32 (each product and each add rounded) against the float64 sum: equal bit
    for bit, rows of the scale-range test (2^-103 .. 2^102) included."""
    for K, centres in ((704, G.range_centres(48)), (2048, None)):
        codes, scales, hi, lo = G.grid_inputs(48, K, 8, 5 + K, centres=centres)
        W = G.weights64(codes, scales)
        Y = R.gemm_sums(W, hi, lo)
        assert np.array_equal(Y.astype(np.float32).astype(np.float64), Y)  # representable
        h32 = hi.astype(np.float32) + lo.astype(np.float32)
        fwd = _fp32_sums(W.astype(np.float32), h32, range(K))
        shuf = _fp32_sums(W.astype(np.float32), h32, np.random.default_rng(1).permutation(K))
        assert np.array_equal(fwd.astype(np.float64), Y) and np.array_equal(shuf.astype(np.float64), Y)


def test_weights64_is_the_rule_s_dequantisation():
    codes, scales, _, _ = G.grid_inputs(16, 64, 32, 3)
    W = G.weights64(codes, scales)
    e = np.repeat(scales.astype(int) - 127, 32, axis=1)
    mag = mx.GRID[codes & 7].astype(np.float64)
    assert np.array_equal(W, np.where(codes & 8, -mag, mag) * np.exp2(e))


def test_library_exports_the_new_entry_points():
    from simplellminference_amd import build, _lib
    build.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sli_prefill_gemm_mxfp4", "sli_model_set_prefill", "sli_tp_group_set_prefill"):
        assert hasattr(L, name), name
    assert [n for n, _ in _lib.PgemmTiling._fields_] == ["BM", "WR", "S", "AT", "PIPE", "SA", "KS"]
