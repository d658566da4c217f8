// mxfp4.h — OCP microscaling FP4 weights (SLI_DT_MXFP4, include/sli.h): e2m1 elements, one e8m0 scale per 32
// consecutive columns, 4.25 bits per weight.
//
// Public layout of a [rows][cols] tensor (cols % 32 == 0): data uint8 [rows][cols / 2], element 2i in bits 3:0 of
// byte i and element 2i + 1 in bits 7:4; a code is sign (bit 3) and magnitude {0, .5, 1, 1.5, 2, 3, 4, 6}[bits 2:0];
// scales uint8 [rows][cols / 32], value 2^(byte - 127). One 16-byte vector of a GEMV lane (gemv.h load_step) is
// exactly one block, so a block never straddles lanes and its scale is one byte per vector.
//
// gfx950 decodes two elements per instruction with the block scale applied in the convert
// (v_cvt_scalef32_pk_f32_fp4: .x = the low nibble, .y = the high nibble of the selected byte — pinned by the
// table-decode test, tests/test_gpu_mxfp4.py); the scale operand is a float whose exponent field is the e8m0 byte.
#pragma once
#include "common.h"

namespace sli {

// weight element type of the GEMV templates: one byte holds two elements
struct mxfp4 {
    uint8_t b;
};

constexpr int kMxBlock = 32;  // elements per scale

template <typename WT>
struct is_mx {
    static constexpr bool value = false;
};
template <>
struct is_mx<mxfp4> {
    static constexpr bool value = true;
};

// bytes of one row of `cols` weights (never cols * sizeof(WT): a 4-bit element is half a byte)
template <typename WT>
__host__ __device__ constexpr size_t wt_row_bytes(size_t cols) {
    return is_mx<WT>::value ? cols / 2 : cols * sizeof(WT);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

template <>
struct Vec16<mxfp4> {
    static constexpr int N = 32;
    // o[8 i + 2 b + {0, 1}] = the two elements of byte b of dword i, times 2^(sbyte - 127)
    __device__ __forceinline__ static void unpack(const u32x4& v, unsigned sbyte, float* o) {
        const float sc = __uint_as_float(sbyte << 23);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[i], sc, 0);
            const f32x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[i], sc, 1);
            const f32x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[i], sc, 2);
            const f32x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[i], sc, 3);
            o[8 * i + 0] = p0.x;
            o[8 * i + 1] = p0.y;
            o[8 * i + 2] = p1.x;
            o[8 * i + 3] = p1.y;
            o[8 * i + 4] = p2.x;
            o[8 * i + 5] = p2.y;
            o[8 * i + 6] = p3.x;
            o[8 * i + 7] = p3.y;
        }
    }
};

// 8 e2m1 codes (element 2i in bits 3:0 of byte i) -> 8 fp16, exact and unscaled, in element order. The high byte
// of the fp16 of magnitude code c is {00, 38, 3C, 3E, 40, 42, 44, 46}[c] (0, .5, 1, 1.5, 2, 3, 4, 6), the low byte 0.
__device__ __forceinline__ u32x4 pg_fp4_to_f16(unsigned w) {
    const unsigned lut_hi = 0x46444240u, lut_lo = 0x3E3C3800u;
    unsigned ev = __builtin_amdgcn_perm(lut_hi, lut_lo, w & 0x07070707u);         // elements 0, 2, 4, 6
    unsigned od = __builtin_amdgcn_perm(lut_hi, lut_lo, (w >> 4) & 0x07070707u);  // elements 1, 3, 5, 7
    ev |= (w & 0x08080808u) << 4;  // the sign bits
    od |= w & 0x80808080u;
    u32x4 r;  // dword i = {00, ev_i, 00, od_i} (selector 0x0c: a zero byte)
    r[0] = __builtin_amdgcn_perm(od, ev, 0x040c000cu);
    r[1] = __builtin_amdgcn_perm(od, ev, 0x050c010cu);
    r[2] = __builtin_amdgcn_perm(od, ev, 0x060c020cu);
    r[3] = __builtin_amdgcn_perm(od, ev, 0x070c030cu);
    return r;
}

// ---------------------------------------------------------------- the quantisation rule (sli.h), in plain C++
// floor(log2(a)) of a finite a > 0, exact (denormals included)
__device__ __forceinline__ int mx_floor_log2(float a) {
    const unsigned u = __float_as_uint(a) & 0x7FFFFFFFu;
    const int ex = (int)(u >> 23);
    return ex ? ex - 127 : (31 - __clz((int)(u & 0x7FFFFFu))) - 149;
}
// scale exponent e of a block whose largest magnitude is amax (byte = e + 127)
__device__ __forceinline__ int mx_block_exp(float amax) {
    if (amax == 0.0f) return 0;
    return max(-127, min(127, mx_floor_log2(amax) - 2));
}
// 4-bit code of w in a block of exponent e: round to nearest on the grid, ties to the even code, saturating
__device__ __forceinline__ unsigned mx_code(float w, int e) {
    const float a = ldexpf(fabsf(w), -e);  // exact scaling
    const unsigned c = (unsigned)(a > 0.25f) + (unsigned)(a >= 0.75f) + (unsigned)(a > 1.25f) +
                       (unsigned)(a >= 1.75f) + (unsigned)(a > 2.5f) + (unsigned)(a >= 3.5f) + (unsigned)(a > 5.0f);
    return c | ((__float_as_uint(w) >> 31) << 3);
}
// table decode (readback, embedding rows: not a hot path)
__device__ __forceinline__ float mx_decode(unsigned code, int e) {
    const unsigned m = code & 7u;
    const float v = m < 4 ? 0.5f * (float)m : (m == 4 ? 2.0f : m == 5 ? 3.0f : m == 6 ? 4.0f : 6.0f);
    return ldexpf((code & 8u) ? -v : v, e);
}
__device__ __forceinline__ float mx_element(const uint8_t* data, const uint8_t* scales, size_t row, int cols, int c) {
    const uint8_t b = data[row * (size_t)(cols / 2) + (c >> 1)];
    const int e = (int)scales[row * (size_t)(cols / kMxBlock) + c / kMxBlock] - 127;
    return mx_decode((c & 1) ? (b >> 4) : (b & 15u), e);
}

// One thread per block of 32: src(row, col) -> 16 data bytes + 1 scale byte at block index blk of the destination.
template <class Src>
__device__ __forceinline__ void mx_quant_block(const Src& src, uint8_t* data, uint8_t* scales, size_t dst_blk) {
    float v[kMxBlock];
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < kMxBlock; ++i) {
        v[i] = src(i);
        amax = fmaxf(amax, fabsf(v[i]));
    }
    const int e = mx_block_exp(amax);
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) w[i] |= mx_code(v[8 * i + k], e) << (4 * k);
    }
    *reinterpret_cast<u32x4*>(data + dst_blk * 16) = u32x4{w[0], w[1], w[2], w[3]};
    scales[dst_blk] = (uint8_t)(e + 127);
}

}  // namespace sli
