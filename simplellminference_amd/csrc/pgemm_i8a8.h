// pgemm_i8a8.h — the int8 prefill GEMM on the integer MFMA of CDNA4 (v_mfma_i32_16x16x64_i8), with the activations as a
// per-token symmetric int8 image (codes int8 [M][K], one fp32 scale per chunk row; the rule: include/sli.h
// sli_prefill_norm_quant_i8). Beside prefill.h's pgemm_kernel, whose int8 format (PgI8) widens the weight bytes to fp16
// and carries the activations as an fp16 hi + lo pair, two v_mfma_f32_16x16x32_f16 per 32 k: here neither operand is
// widened. One MFMA issue multiplies 64 k of a 16 x 16 tile, bytes times bytes, and accumulates in i32, exactly, over
// the whole depth (127^2 K < 2^31: K <= 131072, the host's check). The sums meet fp32 once: acc -> float, times the
// chunk row's scale, then the epilogue of prefill.h with the weight row scales (rscale), unchanged.
//
// Lane layout of the instruction. Lane l = (row l % 16, group kg = l / 16) gives 16 bytes (4 registers) per operand and
// issue, both operands alike. Integer sums do not depend on the order of k, so the kernel is correct for ANY assignment
// of a row's 16-byte chunks to lane groups, as long as A and B use the same one: here group kg of half h (an issue) reads
// the row's logical chunk 4 h + kg, k 64 h + 16 kg .. + 16 of the stage, on both sides. The instruction's own k order is
// therefore not relied on. Read off the hardware with one-hot operands (tools/pgemm_i8a8_lab --layout), for a producer
// that hands operands over in registers: byte j of group g of operand A meets byte j of group g of operand B and no
// other of the 64 (group, byte) slots, for all 64; C[i][n] lands in lane n + 16 (i / 4), register i % 4.
// C is laid out as v_mfma_f32_16x16x32_f16 leaves it (lane l: weight rows 4 (l / 16) .. + 4 of chunk row l % 16), so
// prefill.h's four epilogues serve unchanged.
//
// Stage: 128 k. Per stage the LDS ring holds, all brought by LDS-DMA (lm_dma) and counted by one vmcnt scheme,
//   NA weight images     16 rows x 128 B  (PgI8's image: two 1-KiB pieces of 8 whole lines, lane i -> row i / 8, chunk
//                                          i % 8, chunk swizzle pg_swz(row, 128))
//   PT activation images 16 rows x 128 B  (the same piece shape and swizzle)
// and no scale image: the activation scale is one float per chunk row, loaded after the last stage. The activation image
// is a quarter of the hi/lo pair's (1 byte against 4 per element).
// A fragment read is one ds_read_b128: 16 rows x 16 B per group of 16 lanes, one logical chunk; rows r and r + 1 halve a
// 256-B bank span and the eight row pairs take eight different physical chunks (pg_swz), so the 64 lanes cover the banks
// evenly. Per stage that is two reads per operand and tile, and two MFMAs per tile pair.
// Wave tile: AT weight tiles x PTW position tiles, at least 2 x 2, so every fragment read feeds two or four MFMAs; the
// fragment reads of stage s + 1 are issued ahead of the MFMAs of stage s (two register sets across the stage barrier).
#pragma once
#include "pgemm_mx8.h"  // Mx8SrcF32, Mx8SrcPair, pg8_set_run_kernel

namespace sli {

// ---------------------------------------------------------------- the quantising producers
// the rule of sli.h (place_kernel's for int8 weight rows): s = amax / 127, code = clamp(rint(h / s), -127, 127)
__device__ __forceinline__ unsigned i8a8_code(float h, float s) {
    const float q = s > 0.0f ? rintf(__fdiv_rn(h, s)) : 0.0f;
    return (unsigned)(int)fminf(127.0f, fmaxf(-127.0f, q)) & 0xFFu;
}
__device__ __forceinline__ unsigned i8a8_code4(const float* f, float s) {
    return i8a8_code(f[0], s) | (i8a8_code(f[1], s) << 8) | (i8a8_code(f[2], s) << 16) | (i8a8_code(f[3], s) << 24);
}
__device__ __forceinline__ float i8a8_amax4(const float* f) {
    return fmaxf(fmaxf(fabsf(f[0]), fabsf(f[1])), fmaxf(fabsf(f[2]), fabsf(f[3])));
}
// the row's amax from the threads' own: a wave reduction, then a 4-entry LDS step
__device__ __forceinline__ float i8a8_row_max(float a, float* red) {
    a = wave_max(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// One workgroup per row; thread t holds elements 4 (256 j + t) .. + 4 and stores their 4 codes as one dword. D % 4 == 0.
// NORM: RMSNorm first, pf_norm_split_kernel's structure, operations and summation order (the row in registers, one read
// of x, D <= 8192); h = (x * inv) * w as there, kept in the registers x came in for the code pass.
// Otherwise (any D): two passes over the row, the amax pass and the code pass; the second read comes from L2. (The
// hi / lo pair at D = 11008 does not fit the register budget of the one-pass form.)
template <class Src, bool NORM>
__global__ void __launch_bounds__(256) pf_quant_i8_kernel(Src src, const float* __restrict__ w, int8_t* __restrict__ codes,
                                                         float* __restrict__ scales, int D, float eps) {
    const size_t m = blockIdx.x;
    const int n4 = D / 4;
    __shared__ float red[4], amx[4];
    unsigned* out = reinterpret_cast<unsigned*>(codes + m * D);
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
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
        __syncthreads();
        const float t = red[0] + red[1] + red[2] + red[3];
        const float tep = t / (float)D;      // rms_kernel.cpp:17
        const float rms = sqrtf(tep + eps);  // :18
        const float inv = 1.0f / rms;        // :19
        float a = 0.0f;
#pragma unroll
        for (int j = 0; j < MAXV; ++j)
            if (j * 256 + (int)threadIdx.x < n4) {
                v[j] = make_float4((v[j].x * inv) * wv[j].x, (v[j].y * inv) * wv[j].y, (v[j].z * inv) * wv[j].z,
                                   (v[j].w * inv) * wv[j].w);  // :20-22
                a = fmaxf(a, fmaxf(fmaxf(fabsf(v[j].x), fabsf(v[j].y)), fmaxf(fabsf(v[j].z), fabsf(v[j].w))));
            }
        const float s = __fdiv_rn(i8a8_row_max(a, amx), 127.0f);
        if (threadIdx.x == 0) scales[m] = s;
#pragma unroll
        for (int j = 0; j < MAXV; ++j)
            if (j * 256 + (int)threadIdx.x < n4) {
                const float f[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                out[j * 256 + threadIdx.x] = i8a8_code4(f, s);
            }
    } else {
        float a = 0.0f;
        for (int c = threadIdx.x; c < n4; c += 256) {
            float f[4];
            src.load(m * D + 4 * (size_t)c, f);
            a = fmaxf(a, i8a8_amax4(f));
        }
        const float s = __fdiv_rn(i8a8_row_max(a, amx), 127.0f);
        if (threadIdx.x == 0) scales[m] = s;
        for (int c = threadIdx.x; c < n4; c += 256) {
            float f[4];
            src.load(m * D + 4 * (size_t)c, f);
            out[c] = i8a8_code4(f, s);
        }
    }
}

// ---------------------------------------------------------------- the GEMM
struct PgI8A8In {
    const int8_t* W;  // [N][K] int8 weights (row scales in the epilogue)
    const int8_t* A;  // [M][K] int8 activation codes
    const float* As;  // [M] activation scales
    int N, K, M;      // rows, depth (K % 128 == 0), chunk rows (a multiple of BM)
};

// The tilings are pgemm_mx8.h's Pg8Cfg<BM, WR, WP, S, AT>: a workgroup of WR x WP waves owns BN = 16 AT WR weight rows
// x BM chunk rows; wave (wr, wp) holds the AT x PTW accumulator tiles of weight tiles AT wr .. and position tiles
// PTW wp .. (PTW = BM / 16 / WP). S stages in the ring.
template <class Cfg>
struct PgI8A8Geo {
    static constexpr int BM = Cfg::BM, WR = Cfg::WR, WP = Cfg::WP, S = Cfg::S, AT = Cfg::AT;
    static constexpr int WAVES = WR * WP, THREADS = 64 * WAVES, BN = 16 * AT * WR;
    static constexpr int KS = 128, ROW = 128, IMG = 16 * ROW;  // both operands: 16 rows x 128 B per tile and stage
    static constexpr int NA = AT * WR, PT = BM / 16, PTW = PT / WP;
    static constexpr int A_BYTES = NA * IMG, STAGE = (NA + PT) * IMG;
    // pieces of a stage, 1 KiB each: the weight images' halves, then the activation images'. Every wave issues DPW of
    // them per stage, so one counted vmcnt serves all waves; where the pieces do not divide among the waves the list
    // wraps: a piece is then brought twice (the same bytes to the same place).
    static constexpr int NPA = 2 * NA, NP = 2 * (NA + PT), DPW = (NP + WAVES - 1) / WAVES;
    static constexpr size_t LDS = (size_t)S * STAGE;
    __host__ __device__ static constexpr int piece(int w, int j) { return (w * DPW + j) % NP; }
    static_assert(AT >= 2 && PTW >= 2 && PT % WP == 0 && BM % 16 == 0, "a wave holds at least 2 x 2 tiles");
    static_assert(S >= 2 && S <= 8 && (S - 1) * DPW <= 63, "ring depth (vmcnt counts 63 loads)");
    static_assert(LDS <= 160 * 1024, "LDS");
};

// Where a lane's 16 bytes of piece d come from: the row of the block (weight row 16 tile + r of the row block, or chunk
// row of the position block) and the byte offset in the row's stage-0 slice; a stage advances 128 bytes. Piece d is half
// d & 1 (rows 8 (d & 1) .. + 8) of image d / 2 and lands at byte 1024 d of the stage. Shared with the host.
struct PgI8A8Piece {
    int acts;  // 0: from the weights' array, 1: from the activations'
    int row, off;
};
template <class Geo>
__host__ __device__ constexpr PgI8A8Piece pg_i8a8_piece(int d, int lane) {
    const int o = d < Geo::NPA ? d : d - Geo::NPA;
    const int r = (o & 1) * 8 + (lane >> 3), c = (lane & 7) ^ pg_swz(r, Geo::ROW);
    return {d < Geo::NPA ? 0 : 1, (o >> 1) * 16 + r, c * 16};
}

typedef int pg_i8a8_i4 __attribute__((ext_vector_type(4)));

template <class Epi, class Cfg>
__global__ void __launch_bounds__(64 * Cfg::WR * Cfg::WP) pgemm_i8a8_kernel(PgI8A8In in, Epi epi) {
    using Geo = PgI8A8Geo<Cfg>;
    constexpr int BM = Geo::BM, WR = Geo::WR, S = Geo::S, AT = Geo::AT, NA = Geo::NA, PTW = Geo::PTW, DPW = Geo::DPW;
    extern __shared__ __attribute__((aligned(1024))) char pg_i8a8_smem[];
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
    const unsigned ring = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)pg_i8a8_smem;

    // this wave's pieces: stage-0 source and place in the stage image. A weight tile past the last is the last again
    // (in bounds, never stored).
    const char* src[DPW];
    unsigned dst[DPW];
#pragma unroll
    for (int j = 0; j < DPW; ++j) {
        const int d = Geo::piece(wave, j);
        const PgI8A8Piece p = pg_i8a8_piece<Geo>(d, lane);
        const size_t row = p.acts ? (size_t)(pb * BM + p.row) : (size_t)epi.row(min(rb * NA + (p.row >> 4), nt - 1), p.row & 15);
        src[j] = reinterpret_cast<const char*>(p.acts ? in.A : in.W) + row * (size_t)in.K + p.off;
        dst[j] = (unsigned)(d * 1024);
    }
    auto issue = [&](int s) {
        const unsigned at = ring + (unsigned)((s % S) * Geo::STAGE);
#pragma unroll
        for (int j = 0; j < DPW; ++j) lm_dma(src[j] + (ptrdiff_t)s * Geo::ROW, at + dst[j]);
    };
    pg_i8a8_i4 acc[AT][PTW];
#pragma unroll
    for (int a = 0; a < AT; ++a)
#pragma unroll
        for (int b = 0; b < PTW; ++b) acc[a][b] = pg_i8a8_i4{0, 0, 0, 0};

    // lane l: row / chunk row r16 = l & 15, group kg = l >> 4; half h reads the row's logical chunk 4 h + kg
    const int kg = lane >> 4, r16 = lane & 15;
    const int sw = pg_swz(r16, Geo::ROW);
    const int at0 = r16 * Geo::ROW + ((kg ^ sw) << 4), at1 = r16 * Geo::ROW + (((4 + kg) ^ sw) << 4);
    struct Frags {
        pg_i8a8_i4 a[AT][2], b[PTW][2];
    };
    auto read_frags = [&](const char* st, Frags& f) {
#pragma unroll
        for (int a = 0; a < AT; ++a) {
            const char* img = st + (wr * AT + a) * Geo::IMG;
            f.a[a][0] = *reinterpret_cast<const pg_i8a8_i4*>(img + at0);
            f.a[a][1] = *reinterpret_cast<const pg_i8a8_i4*>(img + at1);
        }
#pragma unroll
        for (int b = 0; b < PTW; ++b) {
            const char* img = st + Geo::A_BYTES + (wp * PTW + b) * Geo::IMG;
            f.b[b][0] = *reinterpret_cast<const pg_i8a8_i4*>(img + at0);
            f.b[b][1] = *reinterpret_cast<const pg_i8a8_i4*>(img + at1);
        }
    };
    // two issues per (weight tile, position tile); the halves are the outer loop, so no two MFMAs in a row share an
    // accumulator
    auto mfmas = [&](const Frags& f) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int b = 0; b < PTW; ++b)
#pragma unroll
                for (int a = 0; a < AT; ++a)
                    acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(f.a[a][h], f.b[b][h], acc[a][b], 0, 0, 0);
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
        read_frags(pg_i8a8_smem + (size_t)(s % S) * Geo::STAGE, f);
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
    // C[i][n] of a 16x16 tile: lane l holds rows 4 (l >> 4) + r, column l & 15. The exact i32 sums become fp32 here
    // (one rounding past 2^24) and take the chunk row's scale; the weight row scales are the epilogue's.
    const int i0 = 4 * (lane >> 4);
#pragma unroll
    for (int b = 0; b < PTW; ++b) {
        const int m = pb * BM + (wp * PTW + b) * 16 + r16;
        const float as = in.As[m];
#pragma unroll
        for (int a = 0; a < AT; ++a) {
            const int t = rb * NA + wr * AT + a;
            if (t >= nt) continue;
            const float v[4] = {(float)acc[a][b][0] * as, (float)acc[a][b][1] * as, (float)acc[a][b][2] * as,
                                (float)acc[a][b][3] * as};
            epi.store(t, i0, m, v);
        }
    }
}

template <class Epi, class Cfg>
hipError_t launch_pgemm_i8a8(const PgI8A8In& in, const Epi& epi, hipStream_t s) {
    using Geo = PgI8A8Geo<Cfg>;
    const int nrb = (in.N + Geo::BN - 1) / Geo::BN;
    const int nrb8 = (nrb + 7) / 8 * 8;
    const dim3 grid(nrb8 * (in.M / Geo::BM));
    hipLaunchKernelGGL((pgemm_i8a8_kernel<Epi, Cfg>), grid, dim3(Geo::THREADS), Geo::LDS, s, in, epi);
    return hipGetLastError();
}

// The tiling per projection role and chunk size (role 0: q/k/v, 1: gate/up, 2: wo / down, 3: logits, on gate/up's
// cells): the fastest of tools/pgemm_i8a8_lab's sweep on the 7B shapes, weights rotated over four copies
// (profiles/i8a8_pgemm_lab.txt). The sweep started from pgemm_mx8.h's cells: the same activation geometry with a weight
// image of twice the bytes, so a stage is (NA + PT) x 2 KiB. With that weight image the 4 x 4 wave tiles of four waves
// lost to eight waves everywhere: 128 x 128 blocks of 2 x 4 waves (4 x 2 tiles each, a 3-deep ring, 96 KiB) for q/k/v at
// 256 and gate/up from 128 (48.8 against 53.8 us at gate/up, M = 256), 128 x 64 blocks of 4 x 2 waves below that; wo /
// down (N = D, few row blocks) keep 64 x 64 blocks of four waves, and M = 32 the 64 x 32 blocks of two.
// f(Pg8Cfg<...>{}) is called with the chosen tiling.
template <class F>
int pg_i8a8_pick(int M, int role, F&& f) {
    if (role == 3) role = 1;
    if (M == 32) return f(Pg8Cfg<32, 2, 1, 4, 2>{});
    if (role == 2) return f(Pg8Cfg<64, 2, 2, 4, 2>{});
    if (M == 64) return role == 0 ? f(Pg8Cfg<64, 2, 2, 4, 2>{}) : f(Pg8Cfg<64, 4, 2, 4, 2>{});
    if (M == 128 && role == 0) return f(Pg8Cfg<64, 4, 2, 4, 2>{});
    return f(Pg8Cfg<128, 2, 4, 3, 4>{});  // q/k/v at 256, gate/up at 128 and 256
}

// the LDS opt-in of every tiling the table can pick for this epilogue
template <class Epi>
hipError_t pg_i8a8_allow_lds_all() {
    hipError_t err = hipSuccess;
    for (int M : kPfSizes)
        for (int role = 0; role < 4; ++role)
            pg_i8a8_pick(M, role, [&](auto cfg) {
                using Cfg = decltype(cfg);
                if (err == hipSuccess)
                    err = hipFuncSetAttribute(reinterpret_cast<const void*>(&pgemm_i8a8_kernel<Epi, Cfg>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)PgI8A8Geo<Cfg>::LDS);
                return 0;
            });
    return err;
}

}  // namespace sli
