"""pgemm_i8a8_kernel (csrc/pgemm_i8a8.h) one launch at a time through sli_prefill_gemm_i8a8, against the int64 product of
the codes times both scales and the reference epilogues of tests/prefill_ref.py (check helpers:
tests/test_gpu_mxfp4_prefill.py). Exact inputs: small codes and power-of-two scales, |acc| < 2^24 (asserted), so every
step after the exact i32 sum is exact in fp32 and the result equals the reference bit for bit. Full-range inputs: codes
reach +-127 on both sides and the scales are no powers of two; what the kernel adds to the exact product is the i32 ->
fp32 conversion and the two scale multiplies, three fp32 roundings: 3 * 2^-24 |acc * ascale * wscale|. (At these depths,
K <= 1024, 127^2 K is still below 2^24 and the conversion itself is exact; the bound does not count on it.)
"""
import numpy as np
import pytest

from tests import prefill_ref as R
from tests import test_gpu_mxfp4_prefill as P
from tests.test_gpu_mxfp4_prefill import tables  # noqa: F401  (the sin / cos fixture)

pytestmark = pytest.mark.gpu

HD = 64


def _exact(N, K, M, seed, top=16):
    """codes in [-top, top]; ascale 2^-3 .. 2^-6, different in neighbouring rows; weight row scales 2^-5 .. 2^-7"""
    r = np.random.default_rng(seed)
    w = r.integers(-top, top + 1, (N, K)).astype(np.int8)
    a = r.integers(-top, top + 1, (M, K)).astype(np.int8)
    a_s = (2.0 ** -(3 + (np.arange(M) + r.integers(0, 4)) % 4)).astype(np.float32)
    ws = (2.0 ** -r.integers(5, 8, N)).astype(np.float32)
    return w, ws, a, a_s


class Ops:
    def __init__(self, torch, w, ws, a, a_s):
        self.torch = torch
        self.dev = [P._t(torch, x) for x in (w, ws, a, a_s)]
        self.N, self.K, self.M = w.shape[0], w.shape[1], a.shape[0]
        self.acc = a.astype(np.int64) @ w.astype(np.int64).T
        self.absacc = int((np.abs(a.astype(np.int64)) @ np.abs(w.astype(np.int64)).T).max())
        self.Y = self.acc.astype(np.float64) * a_s.astype(np.float64)[:, None] * ws.astype(np.float64)[None, :]

    def resid(self, resid=None, pad=0, logits=False):
        from simplellminference_amd import ops
        y = P._sentinel(self.torch, (self.M, self.N + pad), False)
        if logits:
            tl = ops.prefill_gemm_logits_i8a8(*self.dev, y)
        else:
            tl = ops.prefill_gemm_resid_i8a8(*self.dev, y, resid=None if resid is None else P._t(self.torch, resid))
        y = y.cpu().numpy()
        assert P._is_sentinel(y[:, self.N:]).all(), "columns past N were written"
        return y[:, :self.N], tl

    def swiglu(self, silu):
        from simplellminference_amd import ops
        ahi = P._sentinel(self.torch, (self.M, self.N // 2), True)
        alo = P._sentinel(self.torch, (self.M, self.N // 2), True)
        tl = ops.prefill_gemm_gate_up_i8a8(*self.dev, ahi, alo, act_mode=silu)
        return R.joined(ahi.cpu().numpy(), alo.cpu().numpy()), tl

    def qkv(self, tabs, geo, kv, p0, nv, T):
        from simplellminference_amd import ops
        hq, hkv, hd = geo["hq"], geo["hkv"], geo["hd"]
        sin_d, cos_d, _, _ = tabs[hd]
        q = P._sentinel(self.torch, (self.M, hq * hd), False)
        kc = P._sentinel(self.torch, (3, hkv, T, hd), kv == "f16")
        vc = P._sentinel(self.torch, (3, hkv, T, hd), kv == "f16")
        tl = ops.prefill_gemm_qkv_i8a8(*self.dev, q, kc[1], vc[1], sin_d[:T], cos_d[:T], hq, hkv, hd, p0, nv)
        return q.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy(), tl


def _run_role(fails, tag, o, role, tabs, dY, seed):
    """dY None: exact sums (equality where the epilogue is exact); else the sums are known to +- dY."""
    if role == 2:
        resid = R.grid_resid(o.M, o.N, seed) if dY is None else \
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


# ---------------------------------------------------------------- 1. one tile: both operands' lanes, both scales
def test_one_tile_exact(gpu):
    o = Ops(gpu, *_exact(16, 128, 32, 1, top=127))
    assert o.absacc < 2 ** 24 and len(np.unique(o.dev[3].cpu().numpy())) == 4
    for logits in (False, True):
        y, _ = o.resid(pad=16, logits=logits)
        bad = np.argwhere(y != o.Y)
        assert bad.size == 0, f"{len(bad)} of {y.size} sums differ from int64, first (m, row) {bad[:6].tolist()}"


# ---------------------------------------------------------------- 2. exact sums, every cell of the table
@pytest.mark.parametrize("M", [32, 64, 128, 256])
@pytest.mark.parametrize("role", [0, 1, 2, 3])
def test_sums_exact_every_cell(gpu, tables, role, M):  # noqa: F811
    """K = 128 (the ring is longer than the depth), 128 S (one lap) and 128 (S + 1) (the ring wraps); N = one tile and
    BN + 16 (a partial last row block, a padded grid). The q/k/v role takes 3 and 5 heads of 64 rows; role 3 N = 48."""
    torch = gpu
    fails = []
    first = {0: 192, 1: 16, 2: 16, 3: 48}[role]
    tl = _run_role(fails, "first", Ops(torch, *_exact(first, 128, M, 90 + role)), role, tables, None, 1)
    S, BN = tl["S"], 16 * tl["AT"] * tl["WR"]
    assert tl["KS"] == 128 and M % tl["BM"] == 0
    for N in ((first,) if role == 3 else (first, 320 if role == 0 else BN + 16)):
        for K in (128, 128 * S, 128 * (S + 1)):
            o = Ops(torch, *_exact(N, K, M, 1000 * K + 10 * M + role))
            assert o.absacc < 2 ** 24
            assert _run_role(fails, f"N {N} K {K}", o, role, tables, None, K + N) == tl
    assert not fails, f"tiling {tl}:\n" + "\n".join(fails)


# ---------------------------------------------------------------- 3. the full code range, every role
@pytest.mark.parametrize("role,N,K,M", [(0, 320, 640, 64), (1, 288, 640, 128), (2, 272, 1024, 256), (3, 1000, 640, 32)])
def test_full_range(gpu, tables, role, N, K, M):  # noqa: F811
    torch = gpu
    from simplellminference_amd import ops
    r = np.random.default_rng(31 * role + M)
    w32 = (r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    ws = np.abs(w32).max(axis=1) / np.float32(127.0)  # the engine's int8 weight rule (engine.hip place_kernel)
    w = np.clip(np.rint(w32 / ws[:, None]), -127, 127).astype(np.int8)
    a, a_s = ops.prefill_norm_quant_i8(P._t(torch, r.standard_normal((M, K)).astype(np.float32)), None, 0.0)
    o = Ops(torch, w, ws.astype(np.float32), a.cpu().numpy(), a_s.cpu().numpy())
    assert np.abs(o.dev[2].cpu().numpy().astype(np.int32)).max() == 127 and np.abs(w.astype(np.int32)).max() == 127
    fails = []
    _run_role(fails, f"role {role}", o, role, tables, 3 * 2.0 ** -24 * np.abs(o.Y), 5)
    assert not fails, "\n".join(fails)
