// lds_mfma.h — the LDS-DMA / transposed-read / MFMA primitives of the matrix-core kernels (prefill.h, bgemm.h,
// attn_mfma.h, attn_mfma_f8.h), each exactly once, with the hazard each one carries stated where it lives.
//
// The loads here are inline asm, so the compiler neither counts nor drains them (cdna_hip_programming.md §5.7 "What
// hipcc does not do" 1): a kernel that uses lm_dma waits with counted lm_wait_vm and issues no other vector-memory
// load while pieces are in flight; a kernel that uses lm_tr16_read / lm_tr8_read passes every destination to
// lm_tr_landed before its first use.
#pragma once
#include "common.h"

namespace sli {

typedef _Float16 lm_half8 __attribute__((ext_vector_type(8)));
typedef float lm_float4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x32_f16: c += a b, a and b as 8 fp16 per lane
__device__ __forceinline__ lm_float4 lm_mfma(const u32x4& a, const u32x4& b, lm_float4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(lm_half8, a), __builtin_bit_cast(lm_half8, b), c,
                                                  0, 0, 0);
}

// LDS-DMA of one 1-KiB piece: lane i's 16 bytes at gsrc land at LDS byte lds + 16 i. NT: non-temporal (aux 2), for
// bytes read once per step such as K/V cache rows (MI355X_MICROARCH.md nt-weights); what several workgroups read
// keeps the default policy. M0 is written and restored inside the one statement that reads it.
template <bool NT = false>
__device__ __forceinline__ void lm_dma(const void* gsrc, unsigned lds) {
    unsigned keep;
    if constexpr (NT)
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %2\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, off nt\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(gsrc), "s"(lds)
            : "memory");
    else
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %2\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, off\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(gsrc), "s"(lds)
            : "memory");
}
// LDS-DMA of 64 single bytes: lane i's byte at gsrc lands, zero-extended, in the dword at LDS byte lds + 4 i
__device__ __forceinline__ void lm_dma_u8(const void* gsrc, unsigned lds) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_ubyte %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds)
        : "memory");
}
// at most N of this wave's vector-memory loads (DMA pieces) still in flight; vmcnt is 6 bits, N <= 63
template <int N>
__device__ __forceinline__ void lm_wait_vm() {
    static_assert(N >= 0 && N <= 63, "vmcnt is 6 bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// `issued` groups of P pieces each are in flight or landed, in order; wait until the first `needed` have landed,
// leaving at most MAXN later ones in flight
template <int P, int MAXN>
__device__ __forceinline__ void lm_wait_groups(int needed, int issued) {
    if constexpr (MAXN <= 0) {
        lm_wait_vm<0>();
    } else {
        if (needed + (MAXN - 1) < issued)
            lm_wait_vm<MAXN * P>();
        else
            lm_wait_groups<P, MAXN - 1>(needed, issued);
    }
}

// Transposed LDS reads (the A operand of a Vᵀ P MFMA straight from row-major V). b16: per group of 16 lanes a block
// of 4 rows x 16 two-byte columns; b8: 8 rows x 16 one-byte columns (lane layout: attn_mfma_f8.h).
__device__ __forceinline__ uint2 lm_tr16_read(unsigned lds_addr) {
    uint2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(lds_addr) : "memory");
    return v;
}
__device__ __forceinline__ uint2 lm_tr8_read(unsigned lds_addr) {
    uint2 v;
    asm volatile("ds_read_b64_tr_b8 %0, %1" : "=v"(v) : "v"(lds_addr) : "memory");
    return v;
}
// The transposed reads into x have landed (and every other LDS access of the wave: lgkmcnt(0)). An asm load's
// outputs count as written when its statement ends, so without more the compiler may read or copy them above the
// wait: copies of ds_read_b64_tr_b16 results into MFMA operands raced the LDS returns under DMA load (DESIGN.md §9,
// the round-5 fault record). Every destination is therefore an in/out operand of the wait statement itself, which
// pins every use of every x[t] below it. (One statement, not the wait followed by empty statements naming the rest:
// that form is as safe, but hipcc (ROCm 7.2) allocated attn_mfma_kernel<128, ...> 4 to 12 more registers with it.)
template <int N>
__device__ __forceinline__ void lm_tr_landed(uint2 (&x)[N]) {
    static_assert(N == 4 || N == 8 || N == 16, "one operand list per size in use");
#define LM_X4(i) "+v"(x[i]), "+v"(x[i + 1]), "+v"(x[i + 2]), "+v"(x[i + 3])
    if constexpr (N == 4)
        asm volatile("s_waitcnt lgkmcnt(0)" : LM_X4(0) : : "memory");
    else if constexpr (N == 8)
        asm volatile("s_waitcnt lgkmcnt(0)" : LM_X4(0), LM_X4(4) : : "memory");
    else
        asm volatile("s_waitcnt lgkmcnt(0)" : LM_X4(0), LM_X4(4), LM_X4(8), LM_X4(12) : : "memory");
#undef LM_X4
}

// 16-byte chunk swizzles of 32-key fp16 K and V images of 256-byte (head_dim 128) or 128-byte rows (physical chunk =
// logical chunk ^ swizzle(row)): conflict-free ds_read_b128 row reads of K and ds_read_b64_tr_b16 reads of V
__device__ __forceinline__ int lm_swz_k16(int r, int rowb) { return rowb == 256 ? r & 15 : (r >> 1) & 7; }
__device__ __forceinline__ int lm_swz_v16(int r, int rowb) { return rowb == 256 ? (r & 7) << 1 : ((r >> 1) & 3) << 1; }

// (pf_split and am_split3 keep the names their callers in prefill.h and attn_mfma.h use: bodies and names unchanged.)
// fp32 -> fp16 hi + fp16 lo. v is pinned in a register first. Without that the split fuses into the expression that
// produced v: a product a * b contracts into v_fma_mixlo_f16, once for the hi that is stored (the rounded product
// converted) and once more inside the subtraction (the unrounded product). The two hi differ when the product sits
// next to an fp16 tie, lo then has the wrong sign, and hi + lo is one fp16 ulp of hi (2^-11 relative) off: about
// one SwiGLU or attention output in 10^4 (tests/test_gpu_prefill_kernels.py found it).
__device__ __forceinline__ void pf_split(float v, __half& hi, __half& lo) {
    asm("" : "+v"(v));
    hi = __float2half_rn(v);
    lo = __float2half_rn(v - __half2float(hi));
}
// fp32 -> fp16 hi + mid + lo: v - hi - mid - lo is below 2^-33 |v| (or the fp16 subnormal step 2^-24 for |v| <
// 2^-9), so the three exact fp16 products of an MFMA carry the fp32 operand in full (a hi + lo pair carries 22
// bits: measured at C4 position 1, where 32 layers amplify every rounding of the new K/V rows, the pair put the
// logits 1.51e-3 from a float64 restatement against 1.04 - 1.34e-3 for fp32 summation orders)
__device__ __forceinline__ void am_split3(float v, __half& hi, __half& mid, __half& lo) {
    hi = __float2half_rn(v);
    const float r = v - __half2float(hi);  // exact
    mid = __float2half_rn(r);
    lo = __float2half_rn(r - __half2float(mid));
}

}  // namespace sli
