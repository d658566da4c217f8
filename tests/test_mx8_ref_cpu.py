"""tests/mx8_ref.py (the MXFP8 rule in numpy) against blocks worked out by hand from include/sli.h."""
import numpy as np

from tests import mx8_ref as R


def _block(vals):
    b = np.zeros((1, 32), np.float32)
    b[0, :len(vals)] = vals
    return b


def test_hand_written_blocks():
    # amax 3 = 1.5 * 2^1: e = 1 - 8 = -7, byte 120; 3 * 2^7 = 384 = 1.5 * 2^8: exponent field 15, mantissa 4 -> 0x7C;
    # -1.5 * 2^7 = -1.5 * 2^7 -> 0xF4; 3 * 2^-17 * 2^7 = 1.5 subnormal steps of 2^-9: a tie -> the even code 2
    c, s = R.quantize(_block([3.0, -1.5, 0.0, 3.0 * 2.0 ** -17]))
    assert s[0, 0] == 120 and list(c[0, :4]) == [0x7C, 0xF4, 0x00, 0x02]
    # amax 500: e = 0, byte 127; 500 and 449 saturate to 448 (0x7E), 17 is the tie of 16 / 18 -> 16 (even code 0x58)
    c, s = R.quantize(_block([500.0, -449.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10]))
    assert s[0, 0] == 127 and list(c[0, :6]) == [0x7E, 0xFE, 0x58, 0x5A, 0x00, 0x02]
    # a power of two and one fp32 step below it change the scale byte
    assert R.quantize(_block([256.0]))[1][0, 0] == 127 and R.quantize(_block([np.nextafter(np.float32(256), 0)]))[1][0, 0] == 126
    # zero block, -0.0, the lower clamp (denormals) and the top of the range (e = 119)
    c, s = R.quantize(_block([0.0, -0.0]))
    assert s[0, 0] == 127 and list(c[0, :2]) == [0x00, 0x80]
    c, s = R.quantize(_block([2.0 ** -130]))  # -130 - 8 clamps to -127; 2^-130 * 2^127 = 2^-3: exponent field 4
    assert s[0, 0] == 0 and c[0, 0] == 0x20
    c, s = R.quantize(_block([np.float32(3e38)]))
    assert s[0, 0] == 246

