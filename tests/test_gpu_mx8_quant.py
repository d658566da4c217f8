"""pf_quant_mx8_kernel (csrc/pgemm_mx8.h) against the rule in numpy (tests/mx8_ref.py), bit for bit for the plain fp32 and
hi / lo sources; the normed source in the monotone form of "half a code step plus 4 eps32 |h|": under the (equal) block
scale the code lies between the codes of h - d and h + d, d = 4 eps32 |h|, h the float64 norm.
"""
import numpy as np
import pytest

from tests import kv8_ref as f8
from tests import mx8_ref as X
from tests import prefill_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32), (3, 96), (32, 4096), (2, 8192)]


def crafted(M, K, seed=0, f16_range=False):
    """Gaussian blocks with the rule's corners cycled through them; f16_range: without the two ends of the range."""
    r = np.random.default_rng(seed)
    nb = M * K // 32
    lo_k, hi_k = (-6, 5) if f16_range else (-30, 21)
    w = r.standard_normal((nb, 32)).astype(np.float32) * np.exp2(r.integers(lo_k, hi_k, (nb, 1))).astype(np.float32)
    mids = f8.MIDS[[0, 1, 7, 8, 15, 16, 63, 64, 99, 100, 117, 118, 119, 120]].astype(np.float32)
    for i in range(nb):
        sc = np.float32(2.0 ** int(r.integers(-14 if f16_range else -20, -2 if f16_range else 20)))
        kind = i % 9
        u = (r.uniform(-1, 1, 32) * 200.0).astype(np.float32)
        if kind == 0:
            u[:] = 0
            u[0] = 256.0
            u[1:15] = mids
            u[15:29] = -mids
            u[29] = np.nextafter(mids[5], np.float32(0))
            u[30] = np.nextafter(mids[5], np.float32(999))
            u[31] = -np.nextafter(mids[9], np.float32(999))
        elif kind == 1:
            u[:6] = [500.0, 449.0, -464.0, 448.0, 480.0, -511.0]
        elif kind == 2:
            u[4] = -256.0
        elif kind == 3:
            u[9] = np.nextafter(np.float32(256.0), np.float32(0))
        elif kind == 4:
            u[:] = 0
        elif kind == 5:
            u[::3] = -0.0
        elif kind == 6 and not f16_range:
            u, sc = (r.integers(-200, 201, 32) * np.float32(2.0 ** -149)).astype(np.float32), np.float32(1)
        elif kind == 7 and not f16_range:
            u, sc = (r.uniform(-1, 1, 32) * 3e38).astype(np.float32), np.float32(1)
        else:
            continue
        w[i] = u * sc
    return w.reshape(M, K)


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("M,D", SHAPES)
@pytest.mark.parametrize("source", ["f32", "pair"])
def test_codes_and_scales_bit_for_bit(gpu, source, M, D):
    torch = gpu
    from simplellminference_amd import ops
    v = crafted(M, D, seed=M + D, f16_range=source == "pair")
    if source == "pair":
        hi, lo = R.split(v)
        v = hi.astype(np.float32) + lo.astype(np.float32)
        codes, scales = ops.prefill_quant_mx8(_t(torch, hi), _t(torch, lo))
    else:
        codes, scales = ops.prefill_norm_quant_mx8(_t(torch, v), None, 0.0)
    rc, rs = X.quantize(v)
    codes, scales = codes.cpu().numpy(), scales.cpu().numpy()
    assert np.array_equal(scales, rs), np.argwhere(scales != rs)[:4]
    assert np.array_equal(codes, rc), [(i.tolist(), hex(codes[tuple(i)]), hex(rc[tuple(i)])) for i in np.argwhere(codes != rc)[:4]]



@pytest.mark.parametrize("M,D", SHAPES)
def test_normed_source(gpu, M, D):
    torch = gpu
    from simplellminference_amd import ops
    r = np.random.default_rng(7 * M + D)
    x = (r.standard_normal((M, D)) * np.exp2(r.integers(-3, 4, (M, D // 32)).repeat(32, axis=1))).astype(np.float32)
    w = r.uniform(0.5, 1.5, D).astype(np.float32)
    h = R.norm(x, w, 1e-5)
    amax = np.abs(h).reshape(M, D // 32, 32).max(axis=2)
    frac = np.frexp(amax)[0]  # in [.5, 1): a power of two is .5
    assert (np.minimum(frac - 0.5, 1.0 - frac) > 8 * R.EPS32).all(), "a reference block amax sits next to a power of two"
    codes, scales = ops.prefill_norm_quant_mx8(_t(torch, x), _t(torch, w), 1e-5)
    codes, scales = codes.cpu().numpy(), scales.cpu().numpy()
    assert np.array_equal(scales, X.quantize(h.astype(np.float32))[1])
    s = np.ldexp(h, 127 - scales.astype(np.int32).repeat(32, axis=1))  # the float64 norm under the block's scale
    d = 4 * R.EPS32 * np.abs(s)
    got = f8.TABLE64[codes]
    lo, hi = f8.TABLE64[f8.encode(s - d)], f8.TABLE64[f8.encode(s + d)]
    bad = ~((lo <= got) & (got <= hi))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4])
