// pgemm_mx8.h — the MXFP4 prefill GEMM on the block-scaled MFMA of CDNA4 (v_mfma_scale_f32_16x16x128_f8f6f4), with
// the activations as OCP MXFP8 (e4m3 codes, one e8m0 scale per 32 consecutive k; the rule: include/sli.h
// sli_quant_mxfp8). Beside prefill.h's pgemm_kernel, whose MXFP4 format (PgMx) decodes the weights to fp16 and carries
// the activations as an fp16 hi + lo pair: here neither operand is decoded. One MFMA issue multiplies 128 k of a
// 16 x 16 tile, FP4 weights (A) times e4m3 activations (B), and applies both block scales inside the instruction.
//
// Lane layout of the instruction (read off the hardware with one-hot weights, and held by tests/test_gpu_mx8_gemm.py's
// single tile, whose block scales differ on both sides). Lane l = (row l % 16, group kg = l / 16):
//   FP4 operand (4 registers): 16 B = k 32 kg .. + 32 of the row, element 2 i in bits 3:0 of byte i (the public
//     layout): one MX block;
//   e4m3 operand (8 registers): registers 0-3 hold k 16 kg .. + 16, registers 4-7 hold k 64 + 16 kg .. + 16 (the
//     instruction is two 64-k halves of 16 B per lane): chunks kg and 4 + kg of the row's 128-B stage slice;
//   scale register: byte 0 (opsel 0) is the e8m0 byte of (row, k-block kg) of that operand; the hardware applies it
//     by k, to k 32 kg .. + 32, wherever those elements sit in the lanes.
// C is laid out as v_mfma_f32_16x16x32_f16 leaves it (lane l: weight rows 4 (l / 16) .. + 4 of chunk row l % 16), so
// prefill.h's four epilogues serve unchanged. One scale byte per lane and operand: no 2^e dword image and no fp32 FMA
// per C row follow the MFMA.
//
// Stage: 128 k. Per stage the LDS ring holds, all brought by LDS-DMA and counted by one vmcnt scheme,
//   NA weight images     16 rows x 64 B   (1 KiB: one global_load_lds_dwordx4 piece, lane i -> row i / 4, chunk i % 4)
//   PT activation images 16 rows x 128 B  (2 KiB: two pieces of 8 rows, lane i -> row i / 8, chunk i % 8)
//   the weights' scale image [tile][row] of dwords: a row's four scale bytes of the stage ARE one aligned dword of the
//   public [N][K / 32] array (K % 128 == 0), so one global_load_lds_dword piece brings four tiles' scales and lane l
//   reads its one byte, dword (tile, l % 16) byte l / 16, with ds_read_u8: the four lane groups of a row hit one bank
//   entry (a broadcast), no shift and no select follow;
//   the activations' scale image, the same from ascales [M][K / 32].
// The activation image is a quarter of the hi/lo pair's (1 byte against 4 per element), which is what lets every cell
// keep a 3- or 4-deep ring at up to 128 x 128 per workgroup.
// Swizzles (16-byte chunks of an image row, physical chunk = logical ^ swz(row)): a fragment read is ds_read_b128 of
// 16 rows x 16 B per group of 16 lanes, one logical chunk. Weight rows are 64 B, so rows r, r + 4, r + 8, r + 12 start
// in the same 64 banks' quarter: swz = (r >> 2) & 3 (prefill.h pg_mx_swz) gives those four rows four different chunks
// of it, and the 16 lanes cover all 256 B of the bank span once. Activation rows are 128 B, rows r and r + 1 halve a
// span and the eight row pairs need eight different chunks: swz = (r >> 1) & 7 (pg_swz); the lane's two chunks kg,
// 4 + kg are two such reads.
// Wave tile: AT weight tiles x PTW position tiles, at least 2 x 2, so every fragment read feeds two or four MFMAs;
// the fragment and scale reads of stage s + 1 are issued ahead of the MFMAs of stage s (two register sets across the
// stage barrier, as PgCfg::PIPE does per k-block).
#pragma once
#include "prefill.h"

namespace sli {

// ---------------------------------------------------------------- the MXFP8 rule (sli.h), in plain C++
// scale exponent e of a block whose largest magnitude is amax (byte = e + 127); 8 = the exponent of e4m3's 448
__device__ __forceinline__ int mx8_block_exp(float amax) {
    if (amax == 0.0f) return 0;
    return max(-127, min(127, mx_floor_log2(amax) - 8));
}
__device__ __forceinline__ unsigned mx8_code(float v, int e) { return f8e4m3_encode(ldexpf(v, -e)); }  // exact scaling

// ---------------------------------------------------------------- the quantising producers
// The two sources of an activation image: 4 consecutive fp32 of a row, or the fp32 sum of an fp16 hi / lo pair.
struct Mx8SrcF32 {
    const float* x;
    __device__ __forceinline__ void load(size_t i, float* f) const {
        const float4 t = *reinterpret_cast<const float4*>(x + i);
        f[0] = t.x, f[1] = t.y, f[2] = t.z, f[3] = t.w;
    }
};
struct Mx8SrcPair {
    const __half* hi;
    const __half* lo;
    __device__ __forceinline__ void load(size_t i, float* f) const {
        const uint2 h = *reinterpret_cast<const uint2*>(hi + i), l = *reinterpret_cast<const uint2*>(lo + i);
        const __half* hh = reinterpret_cast<const __half*>(&h);
        const __half* ll = reinterpret_cast<const __half*>(&l);
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = __half2float(hh[e]) + __half2float(ll[e]);
    }
};

// One workgroup per row; thread t holds elements 4 (256 j + t) .. + 4, so a block of 32 sits in 8 adjacent lanes of one
// DPP row: its amax is three DPP steps (group_max<8>), no LDS. 4 codes per lane are one 4-byte store, the scale byte
// comes from the block's first lane. D % 32 == 0, so the 8 lanes of a block are active together.
// NORM: RMSNorm first, pf_norm_split_kernel's structure, operations and summation order (the row in registers, one
// read of x, D <= 8192); h = (x * inv) * w as there. (The two kernels are compiled in different translation units, so
// the claim is the same operations in the same order; tests/test_gpu_mx8_quant.py holds this kernel's image against a
// quantisation of the split kernel's hi + lo.)
template <class Src, bool NORM>
__global__ void __launch_bounds__(256) pf_quant_mx8_kernel(Src src, const float* __restrict__ w,
                                                          uint8_t* __restrict__ codes, uint8_t* __restrict__ scales,
                                                          int D, float eps) {
    const size_t m = blockIdx.x;
    const int n4 = D / 4;
    auto emit = [&](int c, const float* f) {  // c: the float4 index in the row
        const float a = group_max<8>(fmaxf(fmaxf(fabsf(f[0]), fabsf(f[1])), fmaxf(fabsf(f[2]), fabsf(f[3]))));
        const int e = mx8_block_exp(a);
        unsigned cw = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) cw |= mx8_code(f[i], e) << (8 * i);
        *reinterpret_cast<unsigned*>(codes + m * D + 4 * (size_t)c) = cw;
        if ((threadIdx.x & 7) == 0) scales[m * (D / 32) + (c >> 3)] = (uint8_t)(e + 127);
    };
    if constexpr (NORM) {
        constexpr int MAXV = 8;  // float4 per thread: D <= 8192
        const float* xr = src.x + m * D;
        float4 v[MAXV], wv[MAXV];
        float ss = 0.0f;
        const float4* w4 = reinterpret_cast<const float4*>(w);
#pragma unroll
        for (int j = 0; j < MAXV; ++j)
            if (j * 256 + (int)threadIdx.x < n4) {
                v[j] = reinterpret_cast<const float4*>(xr)[j * 256 + threadIdx.x];
                wv[j] = w4[j * 256 + threadIdx.x];
                ss += v[j].x * v[j].x + v[j].y * v[j].y + v[j].z * v[j].z + v[j].w * v[j].w;
            }
        ss = wave_sum(ss);
        __shared__ float red[4];
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
        __syncthreads();
        const float t = red[0] + red[1] + red[2] + red[3];
        const float tep = t / (float)D;      // rms_kernel.cpp:17
        const float rms = sqrtf(tep + eps);  // :18
        const float inv = 1.0f / rms;        // :19
#pragma unroll
        for (int j = 0; j < MAXV; ++j)
            if (j * 256 + (int)threadIdx.x < n4) {
                const float f[4] = {(v[j].x * inv) * wv[j].x, (v[j].y * inv) * wv[j].y, (v[j].z * inv) * wv[j].z,
                                    (v[j].w * inv) * wv[j].w};  // :20-22
                emit(j * 256 + threadIdx.x, f);
            }
    } else {
        for (int c = threadIdx.x; c < n4; c += 256) {
            float f[4];
            src.load(m * D + 4 * (size_t)c, f);
            emit(c, f);
        }
    }
}

// codes, scales -> fp32, exact (readback: not a hot path)
static __global__ void dequant_mx8_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                   float* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = ldexpf(f8e4m3_decode(codes[i]), (int)scales[i / kMxBlock] - 127);
}

// the table of one sequence at consecutive positions (prefill_ops.h pf_set_run), written by its 48 threads (mx8.hip asserts the table's size): thread
// 16 a + g writes entry g of array a (sequence, first position, valid rows)
static __global__ void pg8_set_run_kernel(PfSegs* dst, int p0, int nv, int M) {
    const int a = threadIdx.x >> 4, g = threadIdx.x & 15;
    const bool on = g < M / 16;
    const int v = a == 0 ? 0 : a == 1 ? (on ? p0 + 16 * g : 0) : (on ? min(max(nv - 16 * g, 0), 16) : 0);
    reinterpret_cast<int32_t*>(dst)[threadIdx.x] = v;
}

// ---------------------------------------------------------------- the GEMM
struct Pg8In {
    const uint8_t* W;   // mxfp4 data [N][K / 2]
    const uint8_t* Ws;  // e8m0 [N][K / 32], 4-byte aligned
    const uint8_t* A;   // e4m3 codes [M][K]
    const uint8_t* As;  // e8m0 [M][K / 32], 4-byte aligned
    int N, K, M;        // rows, depth (K % 128 == 0), chunk rows (a multiple of BM)
};

// A workgroup of WR x WP waves owns BN = 16 AT WR weight rows x BM chunk rows; wave (wr, wp) holds the AT x PTW
// accumulator tiles of weight tiles AT wr .. and position tiles PTW wp .. (PTW = BM / 16 / WP). S stages in the ring.
template <int BM_, int WR_, int WP_, int S_, int AT_>
struct Pg8Cfg {
    static constexpr int BM = BM_, WR = WR_, WP = WP_, S = S_, AT = AT_;
};

template <class Cfg>
struct Pg8Geo {
    static constexpr int BM = Cfg::BM, WR = Cfg::WR, WP = Cfg::WP, S = Cfg::S, AT = Cfg::AT;
    static constexpr int WAVES = WR * WP, THREADS = 64 * WAVES, BN = 16 * AT * WR;
    static constexpr int KS = 128, A_ROW = 64, B_ROW = 128, A_IMG = 16 * A_ROW, B_IMG = 16 * B_ROW;
    static constexpr int NA = AT * WR, PT = BM / 16, PTW = PT / WP;
    static constexpr int A_BYTES = NA * A_IMG, B_BYTES = PT * B_IMG;
    // pieces of a stage: `big` ones of 1 KiB (weight images, then activation half images), `small` ones of 64 dwords
    // (weight scales, then activation scales; an image is padded to whole pieces)
    static constexpr int NPA = NA, NPB = 2 * PT, NBIG = NPA + NPB;
    static constexpr int NSA = (NA * 16 + 63) / 64, NSB = (PT * 16 + 63) / 64, NSM = NSA + NSB;
    static constexpr int SA_OFF = A_BYTES + B_BYTES, SB_OFF = SA_OFF + NSA * 256, STAGE = SB_OFF + NSB * 256;
    // Every wave issues DPBIG big and DPSM small pieces per stage, so one counted vmcnt serves all waves and a piece's
    // kind is known from its place in the wave's list. Where the pieces do not divide among the waves, the list wraps:
    // a piece is then brought twice (the same bytes to the same place).
    static constexpr int DPBIG = (NBIG + WAVES - 1) / WAVES, DPSM = (NSM + WAVES - 1) / WAVES, DPW = DPBIG + DPSM;
    static constexpr size_t LDS = (size_t)S * STAGE;
    __host__ __device__ static constexpr int big(int w, int j) { return (w * DPBIG + j) % NBIG; }
    __host__ __device__ static constexpr int small(int w, int j) { return (w * DPSM + j) % NSM; }
    static_assert(AT >= 2 && PTW >= 2 && PT % WP == 0 && BM % 16 == 0, "a wave holds at least 2 x 2 tiles");
    static_assert(S >= 2 && S <= 8 && (S - 1) * DPW <= 63, "ring depth (vmcnt counts 63 loads)");
    static_assert(LDS <= 160 * 1024, "LDS");
};

// Where a lane's part of a piece comes from: the row of the block (weight row 16 tile + r of the row block, or chunk
// row of the position block), the byte offset in the row's stage-0 slice, and the bytes a stage advances. Shared with
// the host.
struct Pg8Piece {
    int acts;  // 0: from the weights' array, 1: from the activations'
    int row, off, adv;
};
template <class Geo>
__host__ __device__ constexpr Pg8Piece pg8_big(int d, int lane) {
    if (d < Geo::NPA) {
        const int r = lane >> 2, c = (lane & 3) ^ pg_mx_swz(r, 64);
        return {0, d * 16 + r, c * 16, Geo::A_ROW};
    }
    const int o = d - Geo::NPA, r = (o & 1) * 8 + (lane >> 3), c = (lane & 7) ^ pg_swz(r, 128);
    return {1, (o >> 1) * 16 + r, c * 16, Geo::B_ROW};
}
template <class Geo>
__host__ __device__ constexpr Pg8Piece pg8_small(int d, int lane) {  // dword q of a scale image: (tile, row) = q
    if (d < Geo::NSA) return {0, (d * 64 + lane) % (Geo::NA * 16), 0, 4};
    return {1, ((d - Geo::NSA) * 64 + lane) % (Geo::PT * 16), 0, 4};
}

typedef int pg8_i8 __attribute__((ext_vector_type(8)));

template <class Epi, class Cfg>
__global__ void __launch_bounds__(64 * Cfg::WR * Cfg::WP) pgemm_mx8_kernel(Pg8In in, Epi epi) {
    using Geo = Pg8Geo<Cfg>;
    constexpr int BM = Geo::BM, WR = Geo::WR, S = Geo::S, AT = Geo::AT, NA = Geo::NA, PTW = Geo::PTW;
    constexpr int DPW = Geo::DPW, DPBIG = Geo::DPBIG;
    extern __shared__ __attribute__((aligned(1024))) char pg8_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __builtin_assume(wave >= 0 && wave < Geo::WAVES);
    const int wr = wave % WR, wp = wave / WR;
    const int PB = in.M / BM;
    // workgroups that share a row block run on one XCD (pgemm_kernel's placement; speed only)
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int rb = (slot / PB) * 8 + xcd, pb = slot - (slot / PB) * PB;
    const int nrb = (in.N + Geo::BN - 1) / Geo::BN;
    if (rb >= nrb) return;  // (uniform) padding of the grid to a multiple of 8 row blocks
    const int ns = in.K / Geo::KS;  // whole stages only
    const int nt = in.N >> 4;
    const int sk = in.K / kMxBlock;  // scale bytes per row
    const unsigned ring = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)pg8_smem;

    // this wave's pieces: stage-0 source, bytes per stage, place in the stage image
    const char* src[DPW];
    int adv[DPW];
    unsigned dst[DPW];
#pragma unroll
    for (int j = 0; j < DPW; ++j) {
        const bool sm = j >= DPBIG;
        const int d = sm ? Geo::small(wave, j - DPBIG) : Geo::big(wave, j);
        const Pg8Piece p = sm ? pg8_small<Geo>(d, lane) : pg8_big<Geo>(d, lane);
        size_t row;
        if (p.acts)
            row = (size_t)(pb * BM + p.row);
        else
            row = (size_t)epi.row(min(rb * NA + (p.row >> 4), nt - 1), p.row & 15);
        const uint8_t* base = p.acts ? (sm ? in.As : in.A) : (sm ? in.Ws : in.W);
        const size_t pitch = sm ? (size_t)sk : p.acts ? (size_t)in.K : (size_t)in.K / 2;
        src[j] = reinterpret_cast<const char*>(base) + row * pitch + p.off;
        adv[j] = p.adv;
        dst[j] = sm ? (unsigned)(Geo::SA_OFF + d * 256) : (unsigned)(d * 1024);
    }
    auto issue = [&](int s) {
        const unsigned at = ring + (unsigned)((s % S) * Geo::STAGE);
#pragma unroll
        for (int j = 0; j < DPW; ++j) {
            const char* g = src[j] + (ptrdiff_t)s * adv[j];
            if (j < DPBIG)
                lm_dma(g, at + dst[j]);
            else
                lm_dma_u32(g, at + dst[j]);
        }
    };
    lm_float4 acc[AT][PTW];
#pragma unroll
    for (int a = 0; a < AT; ++a)
#pragma unroll
        for (int b = 0; b < PTW; ++b) acc[a][b] = lm_float4{0.0f, 0.0f, 0.0f, 0.0f};

    // lane l: row / chunk row r16 = l & 15, MX block kg = l >> 4 of the stage
    const int kg = lane >> 4, r16 = lane & 15;
    const int a_at = r16 * Geo::A_ROW + ((kg ^ pg_mx_swz(r16, 64)) << 4);
    const int sb = pg_swz(r16, 128);
    const int b_at0 = r16 * Geo::B_ROW + ((kg ^ sb) << 4), b_at1 = r16 * Geo::B_ROW + (((4 + kg) ^ sb) << 4);
    const int s_at = r16 * 4 + kg;
    struct Frags {
        u32x4 a[AT], b[PTW][2];
        int sa[AT], sb[PTW];
    };
    auto read_frags = [&](const char* st, Frags& f) {
#pragma unroll
        for (int a = 0; a < AT; ++a) {
            const int ti = wr * AT + a;
            f.a[a] = *reinterpret_cast<const u32x4*>(st + ti * Geo::A_IMG + a_at);
            f.sa[a] = *reinterpret_cast<const uint8_t*>(st + Geo::SA_OFF + ti * 64 + s_at);
        }
#pragma unroll
        for (int b = 0; b < PTW; ++b) {
            const int pt = wp * PTW + b;
            const char* img = st + Geo::A_BYTES + pt * Geo::B_IMG;
            f.b[b][0] = *reinterpret_cast<const u32x4*>(img + b_at0);
            f.b[b][1] = *reinterpret_cast<const u32x4*>(img + b_at1);
            f.sb[b] = *reinterpret_cast<const uint8_t*>(st + Geo::SB_OFF + pt * 64 + s_at);
        }
    };
    // one issue per (weight tile, position tile): cbsz 4 = FP4 A (4 registers), blgp 0 = e4m3 B, both scales byte 0
    auto mfmas = [&](const Frags& f) {
#pragma unroll
        for (int b = 0; b < PTW; ++b) {
            const pg8_i8 bv = {(int)f.b[b][0][0], (int)f.b[b][0][1], (int)f.b[b][0][2], (int)f.b[b][0][3],
                               (int)f.b[b][1][0], (int)f.b[b][1][1], (int)f.b[b][1][2], (int)f.b[b][1][3]};
#pragma unroll
            for (int a = 0; a < AT; ++a) {
                const pg8_i8 av = {(int)f.a[a][0], (int)f.a[a][1], (int)f.a[a][2], (int)f.a[a][3], 0, 0, 0, 0};
                acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc[a][b], 4, 0, 0, f.sa[a], 0,
                                                                             f.sb[b]);
            }
        }
    };
    for (int s = 0; s < S - 1 && s < ns; ++s) issue(s);
    // Stage s: this wave's pieces of s landed (it issued whole stages only, DPW loads each, nothing else the counter
    // counts, so at most min(S - 2, ns - 1 - s) later stages are behind them); its fragment reads of s - 1 returned
    // (lgkmcnt(0)), so after the barrier the buffer of s - 1 is free for the DMA of s + S - 1 while those fragments wait
    // in registers for their MFMAs.
    auto enter = [&](int s, Frags& f) {
        pg_wait_stages<DPW>(min(S - 2, ns - 1 - s));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (s + S - 1 < ns) issue(s + S - 1);
        read_frags(pg8_smem + (size_t)(s % S) * Geo::STAGE, f);
    };
    Frags x, y;
    for (int s = 0; s < ns; s += 2) {
        enter(s, x);
        if (s > 0) mfmas(y);
        if (s + 1 < ns) {
            enter(s + 1, y);
            mfmas(x);
        } else {
            mfmas(x);
        }
    }
    if ((ns & 1) == 0) mfmas(y);
    // C[i][n] of a 16x16 tile: lane l holds rows 4 (l >> 4) + r, column l & 15
    const int i0 = 4 * (lane >> 4);
#pragma unroll
    for (int a = 0; a < AT; ++a) {
        const int t = rb * NA + wr * AT + a;
        if (t >= nt) continue;
#pragma unroll
        for (int b = 0; b < PTW; ++b) {
            const int m = pb * BM + (wp * PTW + b) * 16 + r16;
            const float v[4] = {acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]};
            epi.store(t, i0, m, v);
        }
    }
}

template <class Epi, class Cfg>
hipError_t launch_pgemm_mx8(const Pg8In& in, const Epi& epi, hipStream_t s) {
    using Geo = Pg8Geo<Cfg>;
    const int nrb = (in.N + Geo::BN - 1) / Geo::BN;
    const int nrb8 = (nrb + 7) / 8 * 8;
    const dim3 grid(nrb8 * (in.M / Geo::BM));
    hipLaunchKernelGGL((pgemm_mx8_kernel<Epi, Cfg>), grid, dim3(Geo::THREADS), Geo::LDS, s, in, epi);
    return hipGetLastError();
}

// The tiling per projection role and chunk size (role 0: q/k/v, 1: gate/up, 2: wo / down, 3: logits, on gate/up's
// cells): the fastest of tools/pgemm_mx8_lab's sweep on the 7B shapes, weights rotated over four copies
// (profiles/mx8_pgemm_lab.txt). At M = 32 and for wo / down (N = D, few row blocks) 64 x 32 blocks of two waves keep
// the grid full; q/k/v and gate/up take four waves of 2 x 2 tiles at small chunks and 4 x 2 or 4 x 4 tiles (BN = 128:
// a B fragment feeds four MFMAs) from M = 64 (gate/up) / 128 (q/k/v) on; gate/up at M = 256 has enough row blocks
// that 64-row chunk blocks beat 128-row ones (43.2 against 45.5 us). f(Pg8Cfg<...>{}) is called with the chosen tiling.
template <class F>
int pg8_pick(int M, int role, F&& f) {
    if (role == 3) role = 1;
    if (M == 32) return f(Pg8Cfg<32, 2, 1, 4, 2>{});
    if (role == 2) return M == 256 ? f(Pg8Cfg<64, 2, 2, 4, 2>{}) : f(Pg8Cfg<32, 2, 1, 4, 2>{});
    if (M == 64) return role == 0 ? f(Pg8Cfg<64, 2, 2, 4, 2>{}) : f(Pg8Cfg<64, 2, 2, 4, 4>{});
    if ((M == 128) == (role == 0)) return f(Pg8Cfg<64, 2, 2, 4, 4>{});  // q/k/v at 128, gate/up at 256
    return f(Pg8Cfg<128, 2, 2, 4, 4>{});                                // q/k/v at 256, gate/up at 128
}

// the LDS opt-in of every tiling the table can pick for this epilogue
template <class Epi>
hipError_t pg8_allow_lds_all() {
    hipError_t err = hipSuccess;
    for (int M : kPfSizes)
        for (int role = 0; role < 4; ++role)
            pg8_pick(M, role, [&](auto cfg) {
                using Cfg = decltype(cfg);
                if (err == hipSuccess)
                    err = hipFuncSetAttribute(reinterpret_cast<const void*>(&pgemm_mx8_kernel<Epi, Cfg>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)Pg8Geo<Cfg>::LDS);
                return 0;
            });
    return err;
}

}  // namespace sli
