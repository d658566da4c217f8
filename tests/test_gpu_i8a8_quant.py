"""pf_quant_i8_kernel (csrc/pgemm_i8a8.h) against the per-token int8 rule of include/sli.h restated in numpy fp32: scales
bit for bit; codes equal, except that where h / scale lies within one fp32 ulp of a half-integer the neighbouring code is
accepted, for at most 1 element in 10 000 (a condition on the inputs: the float64 quotients of the seeds below were
counted before they were committed, and the test counts them again).
The normed source: pf_norm_split_kernel's hi + lo carries h to 2^-22 only, which cannot decide an amax bit for bit, so h
is restated operation for operation instead, on inputs that make it reproducible: x on an integer grid (|x| <= 32, the
sum of squares is exact in fp32 in any order), then t / D, sqrt(. + eps), 1 / rms, (x * inv) * w, one rounding each. The
split kernel's hi + lo of the same row is held to that h within its 2^-22, which ties the two kernels' norms together.
"""
import numpy as np
import pytest

from tests import prefill_ref as R

pytestmark = pytest.mark.gpu

EPS = np.float32(1e-5)
ZERO_ROW = 5


def _t(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rule(h):
    """h fp32 [M][D] -> codes int8, scales fp32, and the mask of elements whose float64 quotient lies within one fp32
    ulp of a half-integer"""
    h = np.asarray(h, np.float32)
    s = (np.abs(h).max(axis=1) / np.float32(127.0)).astype(np.float32)
    safe = np.where(s > 0, s, np.float32(1.0))[:, None]
    q = (h / safe).astype(np.float32)
    codes = np.where(s[:, None] > 0, np.clip(np.rint(q), -127, 127), 0).astype(np.int8)
    q64 = h.astype(np.float64) / safe.astype(np.float64)
    near = np.abs(np.abs(q64 - np.floor(q64)) - 0.5) <= np.spacing(np.abs(q).astype(np.float32))
    return codes, s, near & (s[:, None] > 0)


def inputs(source, M, D):
    r = np.random.default_rng(1000 * M + D + len(source))
    if source == "norm":
        x = r.integers(-32, 33, (M, D)).astype(np.float32)
        w = r.uniform(0.5, 1.5, D).astype(np.float32)
    else:
        x = (r.standard_normal((M, D)) * np.exp2(r.integers(-3, 4, (M, 1)))).astype(np.float32)
        w = None
    if M > ZERO_ROW:
        x[ZERO_ROW] = 0.0
    return x, w


def norm32(x, w):
    t = (x.astype(np.float64) ** 2).sum(axis=1)
    assert t.max() < 2 ** 24  # integers: the fp32 sum is exact in any order
    tep = (t.astype(np.float32) / np.float32(x.shape[1])).astype(np.float32)
    inv = (np.float32(1.0) / np.sqrt(tep + EPS, dtype=np.float32)).astype(np.float32)
    return ((x * inv[:, None]).astype(np.float32) * w[None, :]).astype(np.float32)


CASES = [(s, M, D) for s in ("f32", "pair", "norm") for D in (128, 4096, 11008) for M in (1, 33)
         if not (s == "norm" and D > 8192)]  # the normed form holds the row in registers: D <= 8192 (sli.h)


@pytest.mark.parametrize("source,M,D", CASES)
def test_codes_and_scales(gpu, source, M, D):
    torch = gpu
    from simplellminference_amd import ops
    x, w = inputs(source, M, D)
    if source == "pair":
        hi, lo = R.split(x)
        h = hi.astype(np.float32) + lo.astype(np.float32)
        codes, scales = ops.prefill_quant_i8(_t(torch, hi), _t(torch, lo))
    elif source == "norm":
        h = norm32(x, w)
        codes, scales = ops.prefill_norm_quant_i8(_t(torch, x), _t(torch, w), float(EPS))
        shi, slo = ops.prefill_norm_split(_t(torch, x), _t(torch, w), float(EPS))
        joined = R.joined(shi.cpu().numpy(), slo.cpu().numpy())
        assert (np.abs(joined - h) <= R.SPLIT_REL * np.abs(h) + R.SPLIT_ABS).all()
    else:
        h = x
        codes, scales = ops.prefill_norm_quant_i8(_t(torch, x), None, 0.0)
    rc, rs, near = rule(h)
    assert near.sum() * 10000 <= near.size, "the inputs break the test's condition"
    codes, scales = codes.cpu().numpy(), scales.cpu().numpy()
    assert np.array_equal(scales.view(np.uint32), rs.view(np.uint32)), np.argwhere(scales != rs)[:4]
    diff = codes != rc
    ok = near & (np.abs(codes.astype(np.int32) - rc.astype(np.int32)) == 1)
    assert not (diff & ~ok).any(), [(i.tolist(), int(codes[tuple(i)]), int(rc[tuple(i)])) for i in np.argwhere(diff & ~ok)[:4]]
    if M > ZERO_ROW:
        assert scales[ZERO_ROW] == 0 and not codes[ZERO_ROW].any()
