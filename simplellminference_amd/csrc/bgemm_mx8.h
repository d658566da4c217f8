// bgemm_mx8.h — the batched decode projection of an MXFP4 model on the block-scaled MFMA of CDNA4
// (v_mfma_scale_f32_16x16x128_f8f6f4): Y[b][row] = sum_k W_fp4[row][k] * A_mx8[b][k] for B <= 8 sequences. Beside
// bgemm.h's bgemm_kernel<.., mxfp4>, which decodes the codes to fp16 in VALU, runs an fp16 MFMA per 32 k and adds the
// block scale with four fp32 FMAs per lane: here one issue multiplies 128 k of a 16-row tile, decodes the FP4 codes
// itself and applies both e8m0 block scales. The activations are OCP MXFP8 (e4m3 codes, one e8m0 scale per 32 k; the
// rule of sli_quant_mxfp8, include/sli.h), quantised by the workgroup while it stages them.
//
// Operands (lane layout: pgemm_mx8.h; lane l = row or column l % 16, group kg = l / 16):
//   A = weights: 16 B per lane and stage, the codes of k 32 kg .. + 32 of tile row l % 16 (one MX block), straight from
//     HBM into registers; the scale register's byte 0 is the e8m0 byte of (row, block kg), loaded beside the data.
//   B = activations: column b < B is sequence b. Registers 0-3: the e4m3 codes of k 16 kg .. + 16, registers 4-7: k
//     64 + 16 kg .. + 16 (two ds_read_b128 of the sequence's 128-B stage row); scale byte of (sequence, block kg) by one
//     ds_read_u8. Columns >= B (8 .. 15 always) are zero codes kept in registers, never read from LDS.
//   C as v_mfma_f32_16x16x32_f16 leaves it, so the per-wave partial tile [16][8], the write-through split hand-off and
//     every epilogue of bgemm.h serve unchanged; there is no hi / lo column pair, so no fold.
//
// Staging. Wave w quantises sequence w / 2: per pass its 64 lanes take 16 MX blocks (2 KiB of one sequence row,
// contiguous), four adjacent lanes one block, 8 k each. The block amax is two DPP steps; exponent and codes come from
// pgemm_mx8.h's mx8_block_exp / mx8_code (the integer codec of pf_quant_mx8_kernel). With a fused RMSNorm the value
// quantised is the fp32 product x * norm_w; the per-sequence 1/rms multiplies the finished sum (it commutes with the
// k-sum), so the codes do not depend on the rms. LDS image: codes [stage][8 sequences][128 B], 16-byte chunks swizzled
// by (sequence >> 1) & 7 (pg_swz: the 8 rows of a B-fragment read hit 8 different 4-bank groups), scales
// [stage][8][4 B]: 1056 B per stage against bgemm.h's 4 KiB per 128 k.
//
// Work split. The 16 waves are wt tiles in flight x wk k-slices (Bg8Plan; bg_mx8_plan decides per launch). Wave
// (ti, ki) streams slice ki of the workgroup's stage range for tiles ti, ti + wt, ... of the workgroup, as one flat
// sequence of (tile, stage) units with kBg8Ring 16-byte loads in flight (the scale bytes travel with them), the
// fragment and scale reads of unit u + 1 issued ahead of the MFMA of unit u. Every wave runs the same number of units
// (rounds x the longest slice), a unit past its slice or past the last tile being a clamped duplicate load whose MFMA
// is skipped, so a shorter slice contributes the stages it has, a wave without stages a zero tile, and nothing is
// read past either image. wk > 1: the wk partial tiles of a round meet in LDS (double-buffered, one barrier per
// round) and one wave per tile sums them in slice order. wk == 1: no barrier and no reduce; with one split the wave
// runs the epilogue's stores for its tile itself and goes on streaming.
#pragma once
#include "bgemm.h"
#include "mx8_api.h"
#include "pgemm_mx8.h"

namespace sli {

struct Bg8Frag {
    u32x4 b0, b1;
    int sb;
};

template <class Epi, bool NORM>
__global__ void __launch_bounds__(kBgThreads) bgemm_mx8_kernel(Bg8In in, Epi epi_in) {
    Epi epi = epi_in;
    extern __shared__ __attribute__((aligned(16))) char bg8_smem[];
    float* red = reinterpret_cast<float*>(bg8_smem);  // [16] the waves' sums of squares
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(bg8_smem + kBgKeysOff);
    int* flag = reinterpret_cast<int*>(bg8_smem + kBgFlagOff);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = in.splits, K = in.K, B = in.B, WK = in.wk, WT = in.wt;
    const int g = blockIdx.x / S, s = blockIdx.x - g * S;
    const int ns = K >> 7;
    const int st0 = (s * ns) / S, nss = ((s + 1) * ns) / S - st0;  // this split's stages
    const int nss_max = (ns + S - 1) / S;
    char* codes = bg8_smem + kBgScratch;                                   // [nss_max][8][128]
    uint8_t* scl = reinterpret_cast<uint8_t*>(codes) + (size_t)nss_max * 1024;  // [nss_max][8][4]
    float* P = reinterpret_cast<float*>(scl + (size_t)nss_max * 32);       // wk > 1: [2][16 waves][16][8]
    float* R = P + (WK > 1 ? 2 * kBgWaves * 128 : 0);                      // [tpw][16][8]
    const int t0 = g * in.tpw;
    const int ntg = min(in.tpw, in.ntiles - t0);  // this workgroup's tiles (uniform)
    const int ti = wave / WK, ki = wave - ti * WK;
    const int ws0 = (ki * nss) / WK, wns = ((ki + 1) * nss) / WK - ws0;  // this wave's stages of the split
    const int cps = max((nss + WK - 1) / WK, 1);                         // units per round (uniform)
    const int rounds = (ntg + WT - 1) / WT;
    const int nunits = rounds * cps;
    const int kg = lane >> 4, c16 = lane & 15;

    if (tid < kBgMaxBatch) keys[tid] = 0ull;
    const unsigned long long t_entry = in.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
    epi.pre_a(t0, ntg, B);

    // ---- the weight stream: unit u = (round u / cps, slice stage u % cps), clamped into the wave's tiles and stages
    auto load_unit = [&](int u, u32x4& w, unsigned& sc) {
        const int uu = min(u, nunits - 1);
        const int r = uu / cps, si = uu - r * cps;
        const int t = t0 + min(r * WT + ti, ntg - 1);
        const int stg = min(st0 + ws0 + min(si, max(wns - 1, 0)), ns - 1);
        const uint8_t *dp, *sp;
        if (in.tiled) {
            const size_t blk = (size_t)t * ns + stg;
            dp = in.w + blk * 1024 + (size_t)lane * 16;
            sp = in.wscale + blk * 64 + lane;
        } else {
            const size_t row = (size_t)epi.row(t, c16);
            dp = in.w + row * (size_t)(K >> 1) + (size_t)stg * 64 + kg * 16;
            sp = in.wscale + row * (size_t)(K >> 5) + (size_t)stg * 4 + kg;
        }
        w = load16<true>(dp);
        sc = __builtin_nontemporal_load(sp);
    };
    u32x4 wr[kBg8Ring];
    unsigned sr[kBg8Ring];

    // ---- 1. stage and quantise. Pass p covers MX blocks 32 p .. + 32 of the split's range for every sequence: wave w
    // takes sequence w / 2, blocks 32 p + 16 (w & 1) + (lane / 4); lane & 3 is the 8-k group of the block.
    const int sq = wave >> 1;
    const int sqc = min(sq, B - 1);
    const int q = lane & 3;
    const int nblk = nss * 4;
    constexpr int NP = 4;  // passes whose loads are issued together
    float4 xa[NP][2];
    float4 wn[NORM ? NP : 1][2];
    float ss = 0.0f;
    auto stage_loads = [&](int p0) {
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            const int bl = (p0 + n) * 32 + 16 * (wave & 1) + (lane >> 2);
            const int gb = min(st0 * 4 + max(min(bl, nblk - 1), 0), (K >> 5) - 1);  // clamped into the row
            const size_t k0 = (size_t)gb * 32 + q * 8;
            const float4* xp = reinterpret_cast<const float4*>(in.x + (size_t)sqc * K + k0);
            xa[n][0] = xp[0];
            xa[n][1] = xp[1];
            if constexpr (NORM) {
                const float4* wp = reinterpret_cast<const float4*>(in.norm_w + k0);
                wn[n][0] = wp[0];
                wn[n][1] = wp[1];
            }
        }
    };
    auto stage_quant = [&](int p0) {
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            const int bl = (p0 + n) * 32 + 16 * (wave & 1) + (lane >> 2);
            const bool live = bl < nblk && sq < B;
            float y[8] = {xa[n][0].x, xa[n][0].y, xa[n][0].z, xa[n][0].w, xa[n][1].x, xa[n][1].y, xa[n][1].z, xa[n][1].w};
            if constexpr (NORM) {
                float v = 0.0f;
#pragma unroll
                for (int e = 0; e < 8; ++e) v += y[e] * y[e];
                ss += live ? v : 0.0f;
                const float wv[8] = {wn[n][0].x, wn[n][0].y, wn[n][0].z, wn[n][0].w,
                                     wn[n][1].x, wn[n][1].y, wn[n][1].z, wn[n][1].w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    y[e] = y[e] * wv[e];
                    asm("" : "+v"(y[e]));  // the rounded fp32 product is what is quantised (no contraction into the codec)
                }
            }
            float a = 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) a = fmaxf(a, fabsf(y[e]));
            a = group_max<4>(a);  // the block's four lanes: two DPP steps
            const int ex = mx8_block_exp(a);
            unsigned c0 = 0, c1 = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c0 |= mx8_code(y[e], ex) << (8 * e);
                c1 |= mx8_code(y[4 + e], ex) << (8 * e);
            }
            if (live) {
                const int st = bl >> 2, kb = bl & 3;
                const int chunk = (kb * 2 + (q >> 1)) ^ pg_swz(sq, 128);
                *reinterpret_cast<uint2*>(codes + (size_t)st * 1024 + sq * 128 + (chunk << 4) + (q & 1) * 8) = make_uint2(c0, c1);
                if (q == 0) scl[st * 32 + sq * 4 + kb] = (uint8_t)(ex + 127);
            }
        }
    };
    // the first pass group's loads, then the ring's first weight loads (vmcnt counts in issue order: the quantiser
    // waits for the activations alone), then the epilogue's second prefetch
    stage_loads(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kBg8Ring; ++i) load_unit(i, wr[i], sr[i]);
    __builtin_amdgcn_sched_barrier(0);
    epi.pre_b();
    stage_quant(0);
    for (int p0 = NP; p0 * 32 < nblk; p0 += NP) {
        stage_loads(p0);
        stage_quant(p0);
    }
    if constexpr (NORM) {
        ss = wave_sum(ss);
        if (lane == 0) red[wave] = ss;
    }
    __syncthreads();  // the image (every wave reads every sequence) and the sums of squares
    float iv = 1.0f;  // this lane's sequence (lane & 7) in every store below
    if constexpr (NORM) {
        const int b = lane & 7;
        const float t = red[2 * b] + red[2 * b + 1];
        const float tep = t / (float)K;         // rms_kernel.cpp:17
        const float rms = sqrtf(tep + in.eps);  // :18
        iv = 1.0f / rms;                        // :19
    }

    const unsigned long long t_staged = in.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
    // ---- 2. stream
    lm_float4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool col_live = c16 < B;
    const int swz = pg_swz(c16, 128);
    const int f_at0 = c16 * 128 + ((kg ^ swz) << 4), f_at1 = c16 * 128 + (((4 + kg) ^ swz) << 4);
    auto read_frag = [&](int u, Bg8Frag& f) {
        const int uu = min(u, nunits - 1);
        const int si = uu - (uu / cps) * cps;
        const int ls = min(ws0 + min(si, max(wns - 1, 0)), nss_max - 1);
        f.b0 = u32x4{0u, 0u, 0u, 0u};
        f.b1 = u32x4{0u, 0u, 0u, 0u};
        f.sb = 127;
        if (col_live) {
            const char* st = codes + (size_t)ls * 1024;
            f.b0 = *reinterpret_cast<const u32x4*>(st + f_at0);
            f.b1 = *reinterpret_cast<const u32x4*>(st + f_at1);
            f.sb = scl[ls * 32 + c16 * 4 + kg];
        }
    };
    auto mfma_unit = [&](int u, const u32x4& w, unsigned sc, const Bg8Frag& f) {
        const int r = u / cps, si = u - r * cps;
        if (si < wns && r * WT + ti < ntg) {  // (uniform per wave)
            const pg8_i8 av = {(int)w[0], (int)w[1], (int)w[2], (int)w[3], 0, 0, 0, 0};
            const pg8_i8 bv = {(int)f.b0[0], (int)f.b0[1], (int)f.b0[2], (int)f.b0[3],
                               (int)f.b1[0], (int)f.b1[1], (int)f.b1[2], (int)f.b1[3]};
            // cbsz 4 = FP4 A (4 registers), blgp 0 = e4m3 B, both scales byte 0
            acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, 4, 0, 0, (int)sc, 0, f.sb);
        }
    };
    auto tile_end = [&](int u) {
        const int r = u / cps, si = u - r * cps;
        if (si != cps - 1) return;  // (uniform per workgroup)
        const int j = r * WT + ti;
        if (WK == 1) {
            if (j < ntg) {
                float* Rj = R + j * 128;
                if ((lane & 8) == 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) Rj[(kg * 4 + e) * 8 + (lane & 7)] = acc[e];
                }
                if (S == 1) {  // the wave's own tile: its stores now. Other lanes of this wave wrote Rj: the writes have
                    // landed before any lane reads (the wave's LDS accesses complete in order; stated, not assumed)
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_wave_barrier();
                    const int i = lane >> 3, b = lane & 7;
                    const float v0 = Rj[i * 8 + b], v1 = Rj[(i + 8) * 8 + b];
                    if (b < B) epi.store(t0 + j, i, b, v0 * iv, v1 * iv, keys);
                }
            }
            acc = lm_float4{0.0f, 0.0f, 0.0f, 0.0f};
            return;
        }
        float* Pb = P + (r & 1) * (kBgWaves * 128);
        if ((lane & 8) == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) Pb[wave * 128 + (kg * 4 + e) * 8 + (lane & 7)] = acc[e];
        }
        acc = lm_float4{0.0f, 0.0f, 0.0f, 0.0f};
        __syncthreads();
        if (ki == (r & (WK - 1)) && j < ntg) {  // tile j's wk slice partials, summed in slice order
            const int i = lane >> 3, b = lane & 7;
            float v0 = 0.0f, v1 = 0.0f;
            for (int w = 0; w < WK; ++w) {
                v0 += Pb[(ti * WK + w) * 128 + i * 8 + b];
                v1 += Pb[(ti * WK + w) * 128 + (i + 8) * 8 + b];
            }
            R[j * 128 + i * 8 + b] = v0;
            R[j * 128 + (i + 8) * 8 + b] = v1;
        }
    };
    Bg8Frag fr[2];
    read_frag(0, fr[0]);
    for (int u = 0; u < nunits; u += kBg8Ring) {
#pragma unroll
        for (int i = 0; i < kBg8Ring; ++i) {
            if (u + i < nunits) {
                read_frag(u + i + 1, fr[(i + 1) & 1]);
                mfma_unit(u + i, wr[i], sr[i], fr[i & 1]);
                if (u + i + kBg8Ring < nunits) load_unit(u + i + kBg8Ring, wr[i], sr[i]);
                tile_end(u + i);
            }
        }
    }
    __syncthreads();
    if (in.stamps && tid == 0) {  // entry, image staged, stream done (and, wk == 1 on one split, stores issued), end
        unsigned long long* sp = in.stamps + (size_t)blockIdx.x * 4;
        sp[0] = t_entry;
        sp[1] = t_staged;
        sp[2] = __builtin_amdgcn_s_memrealtime();
    }

    // ---- 3. epilogue (one split; wk == 1 stored above) or publish + the group's last arriver merges in split order
    // (bgemm.h bgemm_kernel's step 6, statement for statement: its protocol, the vmcnt drain, the counter reset and
    // the sc1 loads, is described there; a change to one belongs in both)
    const int items = ntg * 64;  // (tile, row pair i < 8, sequence slot b < 8)
    if (S == 1) {
        if (WK > 1) {
            for (int it = tid; it < items; it += kBgThreads) {
                const int j = it >> 6, i = (it >> 3) & 7, b = it & 7;
                if (b < B) epi.store(t0 + j, i, b, R[j * 128 + i * 8 + b] * iv, R[j * 128 + (i + 8) * 8 + b] * iv, keys);
            }
        }
    } else {
        for (int e = tid; e < ntg * 128; e += kBgThreads) {
            const int j = e >> 7, r = e & 127;
            __hip_atomic_store(in.ws + ((size_t)(t0 + j) * S + s) * 128 + r, R[e], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains before the arrival
        __syncthreads();
        if (tid == 0) {
            const unsigned prev = __hip_atomic_fetch_add(in.counters + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *flag = prev == (unsigned)(S - 1);
            if (*flag) __hip_atomic_store(in.counters + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (*flag == 0) return;  // uniform
        const float* base = in.ws + (size_t)t0 * S * 128;
        const unsigned bytes = (unsigned)(sizeof(float) * (size_t)ntg * S * 128);
        for (int it = tid; it < items; it += kBgThreads) {
            const int j = it >> 6, i = (it >> 3) & 7, b = it & 7;
            if (b >= B) continue;
            float v0 = 0.0f, v1 = 0.0f;
            for (int sp = 0; sp < S; ++sp) {  // split order: deterministic
                const unsigned o = (unsigned)((j * S + sp) * 128);
                v0 += bg_load_sc1(base, bytes, 4u * (o + i * 8 + b));
                v1 += bg_load_sc1(base, bytes, 4u * (o + (i + 8) * 8 + b));
            }
            epi.store(t0 + j, i, b, v0, v1, keys);
        }
    }
    epi.finish(keys, g, B);
    if (in.stamps && tid == 0) in.stamps[(size_t)blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memrealtime();
}

// Public layout -> the images of Bg8In::tiled, rows in the epilogue's tile order (Epi::row: RoPE pairs, gate/up pairs,
// the last tile's clamped rows). Piece p = (t * K/128 + s) * 64 + l: 16 data bytes and one scale byte. Init-time only.
template <class Epi>
__global__ void __launch_bounds__(256) bg8_tile_kernel(const uint8_t* __restrict__ data, const uint8_t* __restrict__ scales,
                                                        int K, int ntiles, Epi epi, uint4* __restrict__ out,
                                                        uint8_t* __restrict__ sout) {
    const int ns = K / kBg8Stage;
    const size_t n = (size_t)ntiles * ns * 64;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(p & 63);
        const size_t tb = p >> 6;
        const int t = (int)(tb / ns), st = (int)(tb - (size_t)t * ns);
        const size_t row = (size_t)epi.row(t, l & 15);
        out[p] = *reinterpret_cast<const uint4*>(data + row * (size_t)(K >> 1) + (size_t)st * 64 + (l >> 4) * 16);
        sout[p] = scales[row * (size_t)(K >> 5) + (size_t)st * 4 + (l >> 4)];
    }
}

template <class Epi>
hipError_t launch_bg8_tile(const void* data, const void* scales, int K, int ntiles, const Epi& epi, void* out, void* sout,
                           hipStream_t s) {
    if (K % kBg8Stage || !data || !scales || !out || !sout) return hipErrorInvalidValue;
    const size_t n = (size_t)ntiles * (K / kBg8Stage) * 64;
    const int blocks = (int)std::min<size_t>(8192, (n + 255) / 256);
    hipLaunchKernelGGL((bg8_tile_kernel<Epi>), dim3(blocks), dim3(256), 0, s, (const uint8_t*)data, (const uint8_t*)scales, K,
                       ntiles, epi, (uint4*)out, (uint8_t*)sout);
    return hipGetLastError();
}

template <class Epi, bool NORM>
hipError_t bg8_allow_lds() {
    static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&bgemm_mx8_kernel<Epi, NORM>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, kBgLdsMax);
    return e;
}

template <class Epi>
hipError_t launch_bgemm_mx8(const Bg8In& in_, const Epi& epi, const Bg8Plan& p, hipStream_t s) {
    Bg8In in = in_;
    in.ntiles = p.ntiles;
    in.tpw = p.tpw;
    in.splits = p.splits;
    in.wt = p.wt;
    in.wk = p.wk;
    if (bg8_plan_refusal(p.ntiles, in.K, in.norm_w != nullptr, p.tpw, p.splits, p.wt, p.wk)) return hipErrorInvalidValue;
    const dim3 grid(p.groups * p.splits);
    if (in.norm_w)
        hipLaunchKernelGGL((bgemm_mx8_kernel<Epi, true>), grid, dim3(kBgThreads), p.lds, s, in, epi);
    else
        hipLaunchKernelGGL((bgemm_mx8_kernel<Epi, false>), grid, dim3(kBgThreads), p.lds, s, in, epi);
    return hipGetLastError();
}

}  // namespace sli
