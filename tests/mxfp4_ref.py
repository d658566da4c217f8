"""MXFP4 in numpy: the definition of the quantisation rule that include/sli.h documents and the device
quantiser must reproduce bit for bit.

Layout of a [rows, cols] tensor (cols % 32 == 0): data uint8 [rows, cols/2] with element 2i in bits 3:0 of byte i
and element 2i+1 in bits 7:4; a code is the sign in bit 3 and GRID[bits 2:0]; scales uint8 [rows, cols/32], e8m0,
value 2^(byte - 127). Everything is vectorised with a threshold ladder (no per-code distance temporaries).
"""
import numpy as np

BLOCK = 32
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], np.float32)
# the seven midpoints; a tie goes to the even code, so thresholds 0, 2, 4, 6 are exclusive (a > t moves up)
# and 1, 3, 5 inclusive (a >= t moves up)
TIES = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)


def quantize(w):
    """fp32 [rows, cols] -> (codes uint8 [rows, cols] in 0..15, scale bytes uint8 [rows, cols/32])."""
    w = np.ascontiguousarray(w, np.float32)
    rows, cols = w.shape
    assert cols % BLOCK == 0
    b = w.reshape(rows, cols // BLOCK, BLOCK)
    a = np.abs(b)
    amax = a.max(axis=2)
    _, ex = np.frexp(amax)  # amax = m 2^ex, m in [.5, 1): floor(log2(amax)) = ex - 1, exact (denormals too)
    e = np.clip(ex.astype(np.int32) - 1 - 2, -127, 127)
    e = np.where(amax == 0, 0, e).astype(np.int32)
    s = np.ldexp(a, -e[:, :, None]).astype(np.float32)  # exact scaling
    code = np.zeros(s.shape, np.uint8)
    for i, t in enumerate(TIES):
        code += (s > t) if i % 2 == 0 else (s >= t)
    code |= (np.signbit(b).astype(np.uint8) << 3)
    return code.reshape(rows, cols), (e + 127).astype(np.uint8)


def dequantize(codes, scales):
    """(codes [rows, cols], scale bytes [rows, cols/32]) -> fp32 [rows, cols] (exact)."""
    rows, cols = codes.shape
    mag = GRID[codes & 7]
    val = np.where(codes & 8, -mag, mag).astype(np.float32).reshape(rows, cols // BLOCK, BLOCK)
    e = scales.astype(np.int32) - 127
    return np.ldexp(val, e[:, :, None]).astype(np.float32).reshape(rows, cols)


def pack(codes):
    """codes [rows, cols] -> data uint8 [rows, cols/2]: element 2i low nibble, 2i+1 high nibble of byte i."""
    codes = np.asarray(codes, np.uint8)
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack(data):
    """data uint8 [rows, cols/2] -> codes [rows, cols]."""
    data = np.asarray(data, np.uint8)
    out = np.empty((data.shape[0], data.shape[1] * 2), np.uint8)
    out[:, 0::2] = data & 15
    out[:, 1::2] = data >> 4
    return out


def quant_dequant(w):
    """fp32 [rows, cols] -> its MXFP4 round trip as fp32."""
    c, s = quantize(w)
    return dequantize(c, s)


def same_codes(a, b):
    """codes equal modulo the sign of zeros (magnitude 0 may carry either sign bit)."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (((a & 7) == 0) & ((b & 7) == 0))))


def crafted(rows, cols, seed=0):
    """Rows that exercise the rule's corners (cols % 32 == 0, cols >= 64): Gaussian blocks whose maxima spread over
    2^-30 .. 2^20, then — from block 0 of each row on, as far as the row is long — a zero block, a block with one
    denormal, every tie point times the block scale in both signs, amax just under and exactly at a power of two,
    amax = 7.9 2^k (smaller elements land above 5), and -0.0."""
    r = np.random.default_rng(seed)
    nb = cols // BLOCK
    w = r.standard_normal((rows, nb, BLOCK)).astype(np.float32)
    w *= np.exp2(r.integers(-30, 21, size=(rows, nb, 1))).astype(np.float32)
    for i in range(rows):
        k = int(r.integers(-20, 20))
        sc = np.float32(2.0 ** k)
        special = []
        special.append(np.zeros(BLOCK, np.float32))
        d = np.zeros(BLOCK, np.float32)
        d[5] = np.float32(3e-42)
        special.append(d)
        t = np.zeros(BLOCK, np.float32)  # amax 6 sc -> e = k: the ties sit exactly on the midpoints
        t[0] = 6.0
        t[1:8] = TIES
        t[8:15] = -TIES
        t[15] = -6.0
        t[16:23] = np.nextafter(TIES, np.float32(0))
        t[23:30] = np.nextafter(TIES, np.float32(8))
        special.append(t * sc)
        u = (r.uniform(-1, 1, BLOCK) * 3.0).astype(np.float32)  # amax just under 4 sc
        u[3] = np.nextafter(np.float32(4.0), np.float32(0))
        special.append(u * sc)
        p = (r.uniform(-1, 1, BLOCK) * 3.0).astype(np.float32)  # amax exactly 4 sc
        p[7] = -4.0
        special.append(p * sc)
        s79 = (r.uniform(-1, 1, BLOCK) * 7.0).astype(np.float32)  # amax 7.9 sc: e = k, elements above 5 -> 6
        s79[0] = 7.9
        s79[1] = 5.5
        s79[2] = -6.9
        s79[3] = 5.0
        special.append(s79 * sc)
        z = r.standard_normal(BLOCK).astype(np.float32)
        z[::3] = -0.0
        special.append(z * sc)
        for j, blk in enumerate(special[:nb]):
            w[i, (i + j) % nb] = blk
    return w.reshape(rows, cols)
