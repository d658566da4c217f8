"""pgemm_mx8_kernel (csrc/pgemm_mx8.h) one launch at a time through sli_prefill_gemm_mx8, against the float64 product of
the decoded operands and the reference epilogues of tests/prefill_ref.py (check helpers: tests/test_gpu_mxfp4_prefill.py).
Grid inputs: e2m1 codes times integer E4M3 values, block exponents of BOTH sides drawn per block from WINDOW binades, sums
below 2^24 product-grid units (asserted), so the result equals float64 bit for bit in any order. Realistic inputs: SUM_TOL
(|W| @ |A|). (K / 128 + 2) eps32 does not hold, the instruction's internal sum is coarser than fp32: measured worst |err|
/ (|W| @ |A|) on these four cases 16.0, 22.6, 11.7, 15.3 eps32 (one K = 128 issue: 2^-16.5); the factor is
twice the worst, below 2^-16.
"""
import numpy as np
import pytest

from tests import kv8_ref as f8
from tests import mx8_ref as X
from tests import mxfp4_ref as mx
from tests import prefill_ref as R
from tests import test_gpu_mxfp4_prefill as P
from tests.test_gpu_mxfp4_prefill import tables  # noqa: F401  (the sin / cos fixture)

pytestmark = pytest.mark.gpu

WINDOW = 3           # binades of block exponents per side
CW, CA = -7, -2      # centres: weights around 2^-7, activations around 2^-2
HD = 64
SUM_TOL = 2 * 2.70e-6  # twice the measured worst |err| / (|W| @ |A|) of the realistic cases; < 2^-16


def _grid(N, K, M, seed):
    r = np.random.default_rng(seed)
    wc = r.integers(0, 16, (N, K)).astype(np.uint8)
    ws = (CW - 1 + r.integers(0, WINDOW, (N, K // 32)) + 127).astype(np.uint8)
    ac = f8.encode(r.integers(-8, 9, (M, K)).astype(np.float32))  # integers are E4M3 values up to 16
    a_s = (CA - 1 + r.integers(0, WINDOW, (M, K // 32)) + 127).astype(np.uint8)
    return wc, ws, ac, a_s


class Ops:
    def __init__(self, torch, wc, ws, ac, a_s):
        self.torch = torch
        self.dev = [P._t(torch, a) for a in (mx.pack(wc), ws, ac, a_s)]
        self.W = mx.dequantize(wc, ws).astype(np.float64)
        self.A = X.dequantize(ac, a_s)
        self.N, self.M, self.K = wc.shape[0], ac.shape[0], wc.shape[1]
        self.Y = self.A @ self.W.T
        self.absY = np.abs(self.A) @ np.abs(self.W).T

    def units(self):
        step = np.exp2(self.dev[1].cpu().numpy().astype(np.int64).min(axis=1)[None, :] +
                       self.dev[3].cpu().numpy().astype(np.int64).min(axis=1)[:, None] - 254 - 1.0)
        return float((self.absY / step).max())

    def resid(self, resid=None, pad=0, logits=False):
        from simplellminference_amd import ops
        y = P._sentinel(self.torch, (self.M, self.N + pad), False)
        if logits:
            tl = ops.prefill_gemm_logits_mx8(*self.dev, y)
        else:
            tl = ops.prefill_gemm_resid_mx8(*self.dev, y, resid=None if resid is None else P._t(self.torch, resid))
        y = y.cpu().numpy()
        assert P._is_sentinel(y[:, self.N:]).all(), "columns past N were written"
        return y[:, :self.N], tl

    def swiglu(self, silu):
        from simplellminference_amd import ops
        ahi = P._sentinel(self.torch, (self.M, self.N // 2), True)
        alo = P._sentinel(self.torch, (self.M, self.N // 2), True)
        tl = ops.prefill_gemm_gate_up_mx8(*self.dev, ahi, alo, act_mode=silu)
        return R.joined(ahi.cpu().numpy(), alo.cpu().numpy()), tl

    def qkv(self, tabs, geo, kv, p0, nv, T):
        from simplellminference_amd import ops
        hq, hkv, hd = geo["hq"], geo["hkv"], geo["hd"]
        sin_d, cos_d, _, _ = tabs[hd]
        q = P._sentinel(self.torch, (self.M, hq * hd), False)
        kc = P._sentinel(self.torch, (3, hkv, T, hd), kv == "f16")
        vc = P._sentinel(self.torch, (3, hkv, T, hd), kv == "f16")
        tl = ops.prefill_gemm_qkv_mx8(*self.dev, q, kc[1], vc[1], sin_d[:T], cos_d[:T], hq, hkv, hd, p0, nv)
        return q.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy(), tl


def _run_role(fails, tag, o, role, tabs, dY, seed):
    if role == 2:
        resid = R.grid_resid(o.M, o.N, seed) * 2.0 ** (CW + CA) if dY is None else \
            np.random.default_rng(seed).standard_normal((o.M, o.N)).astype(np.float32)
        for res in (resid, None):
            y, tl = o.resid(res, pad=0 if res is not None else 16)
            ref = R.epi_resid(o.Y, None, res)
            tol = 0.0 if dY is None else dY + R.EPS32 * (np.abs(o.Y) + (0.0 if res is None else np.abs(res)))
            P._hold(fails, f"{tag} resid {res is not None}", y, ref, tol)
    elif role == 3:
        y, tl = o.resid(pad=16, logits=True)
        P._hold(fails, f"{tag} logits", y, o.Y, 0.0 if dY is None else dY)
    elif role == 1:
        for silu in (0, 1):
            got, tl = o.swiglu(silu)
            P._check_swiglu(fails, f"{tag} silu {silu}", got, o.Y, dY, silu)
    else:
        hkv = 1
        geo = dict(hq=o.N // HD - 2 * hkv, hkv=hkv, hd=HD)
        p0, nv, T = 3, o.M - 5, o.M - 6  # nv < M, and the last valid rows past T (p0 + m < T ends at m = M - 9)
        for kv in ("f16", "f32"):
            out = o.qkv(tabs, geo, kv, p0, nv, T)
            P._check_qkv(fails, f"{tag} kv {kv}", tabs, out, o.Y, dY, geo, p0, nv, T)
        tl = out[3]
    return tl


# ---------------------------------------------------------------- 1. one tile: the instruction's lane, k and scale layout
def test_one_tile_exact(gpu):
    o = Ops(gpu, *_grid(16, 128, 32, 1))
    assert o.units() < 2 ** 24
    assert len(np.unique(o.dev[1].cpu().numpy())) == WINDOW and len(np.unique(o.dev[3].cpu().numpy())) == WINDOW
    y, _ = o.resid()
    bad = np.argwhere(y != o.Y)
    assert bad.size == 0, f"{len(bad)} of {y.size} sums differ from float64, first (m, row) {bad[:6].tolist()}"


# ---------------------------------------------------------------- 2. exact sums, every cell of the table
@pytest.mark.parametrize("M", [32, 64, 128, 256])
@pytest.mark.parametrize("role", [0, 1, 2, 3])
def test_grid_sums_exact_every_cell(gpu, tables, role, M):  # noqa: F811
    """K = 128 (the ring is longer than the depth), 128 S (one lap) and 128 (S + 1) (the ring wraps); N = one tile and
    BN + 16 (a partial last row block, a padded grid). The q/k/v role takes the smallest N its epilogue admits, 3 and
    5 heads of 64 rows (192: a partial block at BN = 128; 320: five blocks or two and a half); role 3 takes N = 48."""
    torch = gpu
    fails = []
    first = {0: 192, 1: 16, 2: 16, 3: 48}[role]
    tl = _run_role(fails, "first", Ops(torch, *_grid(first, 128, M, 90 + role)), role, tables, None, 1)
    S, BN = tl["S"], 16 * tl["AT"] * tl["WR"]
    assert tl["KS"] == 128 and M % tl["BM"] == 0
    for N in ((first,) if role == 3 else (first, 320 if role == 0 else BN + 16)):
        for K in (128, 128 * S, 128 * (S + 1)):
            o = Ops(torch, *_grid(N, K, M, 1000 * K + 10 * M + role))
            assert o.units() < 2 ** 24
            assert _run_role(fails, f"N {N} K {K}", o, role, tables, None, K + N) == tl
    assert not fails, f"tiling {tl}:\n" + "\n".join(fails)


# ---------------------------------------------------------------- 3. realistic values, every role
@pytest.mark.parametrize("role,N,K,M", [(0, 320, 640, 64), (1, 288, 640, 128), (2, 272, 1024, 256), (3, 1000, 640, 32)])
def test_realistic_values(gpu, tables, role, N, K, M):  # noqa: F811
    torch = gpu
    from simplellminference_amd import ops
    r = np.random.default_rng(31 * role + M)
    w32 = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    data, ws = ops.quant_mxfp4(P._t(torch, w32))
    ac, a_s = ops.quant_mxfp8(P._t(torch, r.standard_normal((M, K)).astype(np.float32)))
    o = Ops(torch, mx.unpack(data.cpu().numpy()), ws.cpu().numpy(), ac.cpu().numpy(), a_s.cpu().numpy())
    fails = []
    assert SUM_TOL <= 2.0 ** -16
    _run_role(fails, f"role {role}", o, role, tables, SUM_TOL * o.absY, 5)
    assert not fails, "\n".join(fails)
