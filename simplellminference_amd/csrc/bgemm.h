// bgemm.h — batched decode projection on MFMA for gfx950: Y[b][row] = sum_k W[row][k] * X[b][k] for a
// batch of B <= 8 sequences decoding in lockstep ("the N=8 skinny GEMM is the only
// place MFMA pays"). It replaces the reference's one-row-per-block matmul_f32_kernel
// (source/kernel/cuda/matmul_kernel.cu:5-38) for B > 1, with the same fused epilogues as the batch-1
// GEMV (gemv.h): RMSNorm prologue (rms_kernel.cpp:5-23), RoPE + K/V cache write (rope_kernel.cpp:22-41),
// SwiGLU (swiglu_kernel.cpp:5-15), residual add (add_kernel.cpp:5-14), logits + argmax keys.
//
// Shape of the work (fp16 weights, fp32 activations, fp32 accumulate):
//   * the weight matrix is cut into 16-row tiles; the epilogue's tile row map lets a tile hold the RoPE
//     partner rows {d, d + hd/2} or the {gate u, up u} rows together (tile rows i and i + 8);
//   * v_mfma_f32_16x16x32_f16: A = 16 weight rows x 32 k straight from HBM (one 16-byte load per lane;
//     cdna_hip_programming.md §3 fragment layout: lane l holds row l&15, k 8(l>>4)..+7), B = 16
//     activation columns: column b < 8 is the fp16 high part of sequence b, column 8 + b its fp16 low
//     part (x - fp16(x)); the fp32 input is carried to ~2^-22 at no MFMA cost (the 8 spare columns of a
//     batch-8 tile) and hi + lo are summed in fp32 after the MFMA;
//   * a workgroup owns `tpw` consecutive tiles and one of `splits` contiguous k-ranges; its 16 waves split
//     the k-range of the current tile, stream it with the next two steps' loads in flight, and their 16
//     partials are reduced in LDS by one wave per tile (round-robin, off the other waves' path);
//   * the activations of the k-range are staged once per workgroup in LDS in the B-fragment layout
//     (lane-linear 16-byte slots: conflict-free ds_read_b128), RMS-normalised per sequence when fused;
//   * splits > 1: per-tile partials are published write-through (sc1) and the group's last-arriving
//     workgroup sums them in split order (deterministic) and runs the epilogue (the hand-off recipe of
//     attention.h, MI355X_MICROARCH.md).
//
// int8 weights (WT = int8_t, per-row symmetric): the same kernel with another A operand. A lane's 8 weights of
// a 16x32 block are 8 bytes in HBM (one 8-byte load per lane and block, half the fp16 path's bytes), turned
// into the fp16 A fragment exactly in registers right before the MFMA (common.h i8x8_to_f16: 2 xor, 4 byte
// permutes, 4 packed subtracts per operand). The row scale is NOT applied to the operand: it multiplies the
// finished fp32 row sum in the epilogue (Epi::rscale; after the per-sequence 1/rms of the NORM plans, before
// anything else the epilogue does). The k-block stays the unit of everything else (per-wave ranges, steps,
// clamped duplicate loads, the plan table), so every K % 32 == 0 and every per-wave block count the fp16
// kernel takes works unchanged, with nothing read past the matrix. The weight type is a template parameter;
// the fp16 instantiations have no int8 code in them.
//
// MXFP4 weights (WT = mxfp4; mxfp4.h: e2m1 codes, one e8m0 scale per 32 columns): one MFMA k-block is exactly one
// MX block, so a (weight row, k-block) pair has one scale. A lane's 8 weights of a 16x32 block are 4 bytes (one
// 4-byte load per lane and block, a quarter of the fp16 path's bytes), decoded to the fp16 A fragment exactly and
// UNSCALED (mxfp4.h pg_fp4_to_f16, the prefill GEMM's decoder). The scale never touches the fp16 operand: the
// kBgU MFMAs of a step run into zeroed tiles of their own, then acc[r] = fma(tile[r], 2^e[r], acc[r]) in fp32 for
// the lane's four C rows 4 (l >> 4) + r, so no block exponent can overflow or flush an fp16. Both activation
// columns (hi: b, lo: 8 + b) take the same row scale, so the lane + 8 fold at the end of a tile stays where it is.
// The scale bytes are loaded beside the data, one byte per lane and block: lane l loads the scale of tile row
// 4 (l >> 4) + (l & 3), and the four lanes of a quad hand each other the four C rows' scales as DPP quad
// broadcasts (VALU operand modifiers, no LDS). Every scale load is unconditional and clamped exactly like the data
// load of the same block, so the loads stay straight-line and nothing is read past either array. The fp16 and
// int8 instantiations have no MXFP4 code in them (if constexpr); the epilogues' rscale stays null.
#pragma once
#include <type_traits>

#include "common.h"
#include "lds_mfma.h"
#include "mxfp4.h"

namespace sli {

constexpr int kBgThreads = 1024;
constexpr int kBgWaves = kBgThreads / 64;
constexpr int kBgMaxBatch = 8;
constexpr int kBgNH = 4;               // staged half-slots (8 k of one sequence) per thread
constexpr int kBgMaxStageK = kBgNH * (kBgThreads / kBgMaxBatch) * 8;  // staged k per sequence <= 4096
constexpr int kBgScratch = 1024;       // bytes: ss partials [16][8] f32, inv [8] f32, keys [8] u64, flag
constexpr int kBgKeysOff = 640;
constexpr int kBgFlagOff = 704;
constexpr int kBgPBytes = 2 * kBgWaves * 16 * 8 * 4;  // double-buffered per-wave tile partials
constexpr int kBgLdsMax = 160 * 1024;
// 16-byte weight loads per lane per step (two steps in flight): 4, or 2 for one-tile plans (a finer
// pipeline over a workgroup's single tile; C4 wo 11.3 -> 10.7 us, TP-8 down 9.3 -> 7.4 us; the multi-tile
// plans lose with 2: down 31.6 -> 33.7 us) — bg_step_width
constexpr int bg_step_width(int tpw) { return tpw == 1 ? 2 : 4; }
// A plan whose waves own 6 or 7 k-blocks of every tile (C4 down: K 14336 over 4 splits, 7; the prefill's
// Llama-2 down: K 11008 over 4 splits, 6) streams each tile as ONE 7-vector step instead of 4 + 3 / 4 + 2
// (clamped duplicates in the second step): C4 down 31.6 -> 29.4 us, 512-token prefill +1.5 %.
#ifndef SLI_BG_U7_FROM
#define SLI_BG_U7_FROM 6
#endif
inline bool bg_seven_blocks(int splits, int K) {
    const int bpw = ((((K >> 5) + splits - 1) / splits) + kBgWaves - 1) / kBgWaves;
    return bpw >= SLI_BG_U7_FROM && bpw <= 7;
}
// The step width (the kBgU instantiation) launch_bgemm runs for a plan: the one place that decides it.
inline int bg_launch_width(bool norm, int tpw, int splits, int K) {
    if (bg_step_width(tpw) == 2) return 2;
    return !norm && bg_seven_blocks(splits, K) ? 7 : 4;
}

struct BgIn {
    const float* x;       // [B][K] fp32 activations
    const float* norm_w;  // fused RMSNorm weight [K], or nullptr
    float eps;
    int K;
    int B;
    int ntiles;           // 16-row output tiles
    int tpw;              // tiles per workgroup
    int splits;           // k-ranges (workgroups per tile group)
    float* ws;            // splits > 1: partials [ntiles][splits][16][8]
    unsigned* counters;   // splits > 1: [groups] arrival counters, zero between launches
    unsigned long long* stamps = nullptr;  // diagnostic (tools/bgemm_lab): per-workgroup s_memrealtime x4
    // W in the fragment layout (bg_tile_kernel): tile t's k-block kb is 1 KiB at ((t * K/32) + kb) * 1024, lane l's
    // 16-byte A operand at l * 16 — one wave load is one contiguous KiB (8 full 128-B lines) instead of 16 rows x
    // 64 B (16 half lines). 0: W row-major [rows][K] (the op-level entry, tools/bgemm_lab).
    // int8: the same order at half the size — block kb of tile t is 512 B at ((t * K/32) + kb) * 512, lane l's 8
    // bytes W[row(t, l & 15)][32 kb + 8 (l >> 4) .. + 7] at l * 8: one wave load is one contiguous, fully used run
    // of four 128-B lines (row-major: 16 rows x 32 B, 16 quarter lines), and a wave's consecutive blocks are
    // consecutive in memory, so the loads of one step cover one run of kBgU * 512 B. (Pairing two k-blocks into
    // 16-byte lane loads would tie the image to the plan: a wave's first block is odd or even with the split.)
    // mxfp4: two images. Data: block kb of tile t is 256 B at ((t * K/32) + kb) * 256, lane l's 4 bytes (the codes of
    // W[row(t, l & 15)][32 kb + 8 (l >> 4) .. + 7]) at l * 4: one wave load is two full 128-B lines. Scales: 16 B per
    // (tile, k-block) at ((t * K/32) + kb) * 16, byte i the e8m0 scale of row(t, i) (a clamped row carries its real
    // row's scale); lane l loads byte 4 (l >> 4) + (l & 3). A wave's consecutive blocks are consecutive in both
    // images. tiled = 0: data [rows][K/2] and scales [rows][K/32] in the public layout of sli.h.
    int tiled = 0;
    const uint8_t* wscale = nullptr;  // mxfp4 only: the e8m0 block scales, in the layout `tiled` names
};

// ---------------------------------------------------------------- host-side plan
struct BgPlan {
    int ntiles = 0, tpw = 1, splits = 1, groups = 0;
    size_t lds = 0;
};

inline size_t bg_lds_bytes(int K, int splits, int tpw) {
    const int nkb = K / 32;
    const int kbs = (nkb + splits - 1) / splits;
    return (size_t)kBgScratch + (size_t)kbs * 1024 + kBgPBytes + (size_t)tpw * 512;
}

// (tiles per workgroup, k-splits) for a [16*ntiles x K] weight: about one workgroup per CU, the activation
// staging amortised over several tiles (B*K/splits*4 bytes from L2 per workgroup, plus B*K*4 for the
// fused RMS over the full row), the LDS image within 160 KiB. Cost in units of one 16x32 fp16 weight
// block (1 KiB of HBM); L2 bytes priced at a quarter of HBM bytes.
inline BgPlan bg_plan(int ntiles, int K, int B, bool norm, int cus = 256) {
    const int nkb = K / 32;
    BgPlan best;
    double best_cost = 1e30;
    for (int s = 1; s <= 16; ++s) {
        if (s > 1 && nkb / s < kBgWaves) break;  // every wave keeps at least one block per tile
        // the fused RMS needs the whole row in one workgroup (measured round 2: splitting k for the fused-
        // RMS plans, each split's sum of squares merged by the last arriver, was correct but slower — at
        // K 4096 a split leaves each wave one partly-filled step per tile and a barrier per step)
        if (norm && s > 1) break;
        const int kbs = (nkb + s - 1) / s;
        if (kbs * 32 > kBgMaxStageK) continue;  // staging registers
        for (int tpw = 1; tpw <= 64; ++tpw) {
            if (bg_lds_bytes(K, s, tpw) > (size_t)kBgLdsMax) break;
            const int groups = (ntiles + tpw - 1) / tpw;
            const int wgs = groups * s;
            const int rounds = (wgs + cus - 1) / cus;
            double per_wg = (double)tpw * kbs + 0.25 * kbs * B / 8.0 + 40.0;
            if (norm) per_wg += 0.25 * nkb * B / 8.0;
            if (s > 1) per_wg += 20.0 + 0.5 * s * tpw;
            const double cost = rounds * per_wg;
            if (cost < best_cost - 1e-9) {
                best_cost = cost;
                best.ntiles = ntiles;
                best.tpw = tpw;
                best.splits = s;
                best.groups = groups;
                best.lds = bg_lds_bytes(K, s, tpw);
            }
            if (groups == 1) break;
        }
    }
    return best;
}

// device workspace of a plan: split partials (256-B aligned), then one arrival counter per group
inline size_t bg_part_bytes(const BgPlan& p) {
    return p.splits > 1 ? (((size_t)p.ntiles * p.splits * 128 * sizeof(float) + 255) & ~(size_t)255) : 0;
}
inline size_t bg_ws_bytes(const BgPlan& p) { return bg_part_bytes(p) + sizeof(unsigned) * (size_t)p.groups + 256; }

// ---------------------------------------------------------------- device side
__device__ __forceinline__ float bg_load_sc1(const float* base, unsigned bytes, unsigned off) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 16 /* sc1 */));
}

// fp32 -> (fp16 hi, fp16 lo), hi + lo == v to ~2^-22 relative
__device__ __forceinline__ void bg_split8(const float* y, u32x4& hi, u32x4& lo) {
    unsigned h[4], l[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const _Float16 h0 = (_Float16)y[2 * p], h1 = (_Float16)y[2 * p + 1];
        const _Float16 l0 = (_Float16)(y[2 * p] - (float)h0), l1 = (_Float16)(y[2 * p + 1] - (float)h1);
        h[p] = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
        l[p] = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
    }
    hi = u32x4{h[0], h[1], h[2], h[3]};
    lo = u32x4{l[0], l[1], l[2], l[3]};
}

// bytes of a lane's 8 weights of one 16x32 block: 16 (fp16), 8 (int8), 4 (mxfp4)
template <typename WT>
__host__ __device__ constexpr size_t bg_lane_bytes() {
    return is_mx<WT>::value ? 4 : 8 * sizeof(WT);
}

// mxfp4: the fp32 scale of C row r of a lane from the quad's scale bytes (QP: quad_perm [r, r, r, r]). The scale is the
// float whose exponent field is the e8m0 byte: bytes 1 .. 254 are the normal numbers 2^-126 .. 2^127. Byte 0 is
// 2^-127, an fp32 subnormal (word 0x00400000), not the zero that byte << 23 would give: the unsigned max supplies
// it (fp32 denormals are kept, so the product is the exact one whenever it is representable). Byte 255 (the
// format's NaN) becomes an infinity, and the row sum a NaN or an infinity.
template <int QP>
__device__ __forceinline__ float bg_mx_scale(unsigned sbyte) {
    const unsigned b = (unsigned)__builtin_amdgcn_mov_dpp((int)sbyte, QP, 0xF, 0xF, true);
    return __uint_as_float(max(b << 23, 0x00400000u));
}

// Epilogue contract (a mutable copy per thread):
//   row(t, i)                   weight row of tile t's row i (i < 16), always a valid row (clamped)
//   store(t, i, b, v0, v1, kl)  final sums of tile rows i (< 8) and i + 8 for sequence b; kl = the
//                               workgroup's per-sequence argmax keys in LDS
//   finish(kl, group, B)        once per workgroup that ran stores, after all of them
//   pre_a(t0, ntg, B), pre_b()  the epilogue's own inputs for this thread's first item (it = tid: tile t0 +
//                               (it >> 6), row pair (it >> 3) & 7, sequence it & 7), issued before the
//                               activation loads (pre_a) and right after the first weight steps (pre_b, for
//                               loads that depend on pre_a's), so they land during the stream instead of
//                               costing a round trip after it
template <class Epi, bool NORM, int kBgU = 4, typename WT = __half>
__global__ void __launch_bounds__(kBgThreads) bgemm_kernel(const WT* __restrict__ W, BgIn in, Epi epi_in) {
    static_assert(std::is_same<WT, __half>::value || std::is_same<WT, int8_t>::value || is_mx<WT>::value,
                  "fp16, int8 or mxfp4 weights");
    constexpr bool I8 = std::is_same<WT, int8_t>::value;
    constexpr bool MX = is_mx<WT>::value;
    constexpr size_t ES = sizeof(WT);  // fp16, int8: a lane's A operand of one k-block: 8 elements = 8 * ES bytes
    using WV = typename std::conditional<MX, unsigned, typename std::conditional<I8, u32x2, u32x4>::type>::type;
    Epi epi = epi_in;
    extern __shared__ __attribute__((aligned(16))) char bg_smem[];
    float* red = reinterpret_cast<float*>(bg_smem);  // [16][8]
    float* inv = red + kBgWaves * 8;                 // [8]
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(bg_smem + kBgKeysOff);
    int* flag = reinterpret_cast<int*>(bg_smem + kBgFlagOff);
    u32x4* img = reinterpret_cast<u32x4*>(bg_smem + kBgScratch);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = in.splits, K = in.K, B = in.B;
    const int g = blockIdx.x / S, s = blockIdx.x - g * S;
    const int nkb = K >> 5;
    const int kb0 = (s * nkb) / S, nkbs = ((s + 1) * nkb) / S - kb0;  // this split's 32-k blocks
    const int kbs_max = (nkb + S - 1) / S;
    float* P = reinterpret_cast<float*>(bg_smem + kBgScratch + (size_t)kbs_max * 1024);  // [2][16 waves][16][8]
    float* R = P + 2 * kBgWaves * 128;                                                 // [tpw][16][8]
    const int t0 = g * in.tpw;
    const int ntg = min(in.tpw, in.ntiles - t0);  // this workgroup's tiles (uniform)
    const int wb0 = kb0 + (wave * nkbs) / kBgWaves;  // this wave's blocks of every tile
    const int wnb = kb0 + ((wave + 1) * nkbs) / kBgWaves - wb0;
    const int per_wave_max = (nkbs + kBgWaves - 1) / kBgWaves;
    const int cpt = max((per_wave_max + kBgU - 1) / kBgU, 1);  // steps per tile (uniform)
    const int nsteps = ntg * cpt;

    if (tid < kBgMaxBatch) keys[tid] = 0ull;
    const unsigned long long t_entry = in.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
    epi.pre_a(t0, ntg, B);

    // ---- 1. activation staging loads, issued first (s_waitcnt vmcnt counts in issue order). Thread t
    // stages sequence b = t & 7 at the 8-k groups (t >> 3) + 128 n: the 8 lanes of a group write 8
    // consecutive 16-byte image slots (conflict-free ds_write_b128), the loads stay 32 B per lane.
    // Without the fused RMS (wo, down) nothing needs the whole row, so every WAVE stages only its own
    // blocks [wb0, wb0 + wnb) (the blocks its MFMAs read, for every tile of the workgroup) and starts
    // streaming as soon as they land: no workgroup barrier behind the slowest wave's activations (the
    // B*K*4-byte image is pulled through L2 by 256 workgroups at once; profiles/r04_bgemm_lab_*).
    // Lane l: sequence l >> 3, block 2n + ((l >> 2) & 1), 8-k group l & 3: 8 lanes read 256
    // contiguous bytes of one sequence row.
    // With the fused RMS the norm is split the same way: the image holds x * w (rms_kernel.cpp:20-22
    // without the per-sequence 1/rms), every wave adds its blocks' sum of squares to LDS, and the
    // per-sequence 1/rms (:12-19) multiplies the finished row sums in the epilogue: a per-sequence scalar
    // commutes with the k-sum. NORM plans have one split (bg_plan), so the waves' blocks cover the row.
    const int sb = lane >> 3;
    const bool seq_live = sb < B;
    const int sbc = min(sb, B - 1);
    const int wq = lane & 3, wbo = (lane >> 2) & 1;  // per-wave staging: 8-k group, block offset
    float4 xa[kBgNH][2];
    float4 wn[NORM ? kBgNH : 1][2];
#ifdef BG_LAB_NOSTAGE  // tools/bgemm_lab only: no activation loads (an upper bound on what a ready image saves)
    constexpr bool kStage = false;
#else
    constexpr bool kStage = true;
#endif
#pragma unroll
    for (int n = 0; n < kBgNH; ++n) {
        const int blk = wb0 + max(min(2 * n + wbo, wnb - 1), 0);  // clamped into the row, never a branch
        const int k8 = min(blk, nkb - 1) * 4 + wq;
        const float4* xp = reinterpret_cast<const float4*>(in.x + (size_t)sbc * K + (size_t)k8 * 8);
        xa[n][0] = kStage ? xp[0] : make_float4(0.f, 0.f, 0.f, 0.f);
        xa[n][1] = kStage ? xp[1] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (NORM && kStage) {
#pragma unroll
        for (int n = 0; n < kBgNH; ++n) {
            const int blk = wb0 + max(min(2 * n + wbo, wnb - 1), 0);
            const float4* wp = reinterpret_cast<const float4*>(in.norm_w + (size_t)(min(blk, nkb - 1) * 4 + wq) * 8);
            wn[n][0] = wp[0];
            wn[n][1] = wp[1];
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- 2. the first two weight steps
    const size_t row_bytes = (size_t)K * ES;
    const int q8 = (lane >> 4) * 8;  // this lane's k offset inside a 32-k block
    const size_t bstride = in.tiled ? 512 * ES : 32 * ES;  // bytes between a lane's consecutive k-blocks
    // mxfp4: the tile row whose scale this lane loads (its quad holds the scales of the lane's four C rows)
    const int srow = (lane >> 4) * 4 + (lane & 3);
    auto load_step = [&](int k, WV(&w)[kBgU], unsigned(&ws)[MX ? kBgU : 1]) {
        const int kk = min(k, nsteps - 1);
        const int j = kk / cpt, c = kk - j * cpt;
        if constexpr (MX) {
            // 4 data bytes and 1 scale byte per lane and block. 32-bit block offsets (at most 256 B x K / 32 blocks),
            // and a block's scale offset is its data offset / 16 in both layouts (256 and 16 bytes per block tiled,
            // 16 and 1 row-major): that keeps the widest epilogue within the scalar registers (no scratch).
            const unsigned mstride = in.tiled ? 256u : 16u;
            const char* base;
            const uint8_t* sbase;
            if (in.tiled) {
                base = reinterpret_cast<const char*>(W) + (size_t)(t0 + j) * nkb * 256 + (size_t)lane * 4;
                sbase = in.wscale + (size_t)(t0 + j) * nkb * 16 + srow;
            } else {
                base = reinterpret_cast<const char*>(W) + (size_t)epi.row(t0 + j, lane & 15) * (size_t)(K >> 1) +
                       (size_t)(lane >> 4) * 4;
                sbase = in.wscale + (size_t)epi.row(t0 + j, srow) * nkb;
            }
#pragma unroll
            for (int u = 0; u < kBgU; ++u) {
                const int bi = wb0 + min(c * kBgU + u, max(wnb - 1, 0));
                const unsigned off = (unsigned)bi * mstride;
                w[u] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(base + off));
                ws[u] = __builtin_nontemporal_load(sbase + (off >> 4));
            }
        } else {
            const char* base;
            if (in.tiled) {
                base = reinterpret_cast<const char*>(W) + (size_t)(t0 + j) * nkb * (512 * ES) + (size_t)lane * (8 * ES);
            } else {
                const int row = epi.row(t0 + j, lane & 15);
                base = reinterpret_cast<const char*>(W) + (size_t)row * row_bytes + (size_t)q8 * ES;
            }
#pragma unroll
            for (int u = 0; u < kBgU; ++u) {
                const int bi = wb0 + min(c * kBgU + u, max(wnb - 1, 0));
                if constexpr (I8)
                    w[u] = load8<true>(base + (size_t)bi * bstride);
                else
                    w[u] = load16<true>(base + (size_t)bi * bstride);
            }
        }
    };
    WV wa[kBgU], wb[kBgU];  // (a third step in flight measured slower: C4 1660 -> 1546 tok/s)
    unsigned sa[MX ? kBgU : 1], sb_[MX ? kBgU : 1];  // mxfp4: the steps' scale bytes
    load_step(0, wa, sa);
    load_step(1, wb, sb_);
    __builtin_amdgcn_sched_barrier(0);
    epi.pre_b();

    // ---- 3./4. this wave's blocks into LDS as B fragments (hi: column b, lo: 8 + b), visible to the
    // wave's own later reads after lgkmcnt(0); NORM: x * w staged, this wave's sum of x^2 to red[wave][b]
    float ss = 0.0f;
#pragma unroll
    for (int n = 0; n < kBgNH; ++n) {
        const int bw = 2 * n + wbo;
        float y[8] = {xa[n][0].x, xa[n][0].y, xa[n][0].z, xa[n][0].w, xa[n][1].x, xa[n][1].y, xa[n][1].z, xa[n][1].w};
        if constexpr (NORM) {
            float v = 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) v += y[e] * y[e];
            ss += bw < wnb ? v : 0.0f;
            const float wv[8] = {wn[n][0].x, wn[n][0].y, wn[n][0].z, wn[n][0].w,
                                 wn[n][1].x, wn[n][1].y, wn[n][1].z, wn[n][1].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) y[e] = y[e] * wv[e];
        }
        if (seq_live && bw < wnb) {
            u32x4 hi, lo;
            bg_split8(y, hi, lo);
            const int ib = wb0 - kb0 + bw;
            img[ib * 64 + wq * 16 + sb] = hi;
            img[ib * 64 + wq * 16 + 8 + sb] = lo;
        }
    }
    if constexpr (NORM) {
        ss = group_sum<8>(ss);  // the 8 lanes of one sequence
        if ((lane & 7) == 0) red[wave * 8 + sb] = ss;  // read after the stream's final barrier
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();

    const unsigned long long t_staged = in.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
    // ---- 5. stream the tiles
    lm_float4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const u32x4* wimg = img + (size_t)(wb0 - kb0) * 64 + lane;
    auto mfma_step = [&](int k, const WV(&w)[kBgU], const unsigned(&ws)[MX ? kBgU : 1]) {
        const int c = k - (k / cpt) * cpt;
        if constexpr (MX) {
            // the step's MFMAs into zeroed tiles of their own, then the scaled adds (no MFMA waits on an FMA)
            lm_float4 tile[kBgU];
#pragma unroll
            for (int u = 0; u < kBgU; ++u) {
                tile[u] = lm_float4{0.0f, 0.0f, 0.0f, 0.0f};
                if (c * kBgU + u < wnb) tile[u] = lm_mfma(pg_fp4_to_f16(w[u]), wimg[(size_t)(c * kBgU + u) * 64], tile[u]);
            }
#pragma unroll
            // (unconditional: a block past the wave's range left its tile zero, and its clamped duplicate's scale
            // is that of a real block of the same rows, so it adds +0 to a sum that is never -0)
            for (int u = 0; u < kBgU; ++u) {
                acc[0] = fmaf(tile[u][0], bg_mx_scale<0x00>(ws[u]), acc[0]);
                acc[1] = fmaf(tile[u][1], bg_mx_scale<0x55>(ws[u]), acc[1]);
                acc[2] = fmaf(tile[u][2], bg_mx_scale<0xAA>(ws[u]), acc[2]);
                acc[3] = fmaf(tile[u][3], bg_mx_scale<0xFF>(ws[u]), acc[3]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < kBgU; ++u) {
                const int r = c * kBgU + u;
                if constexpr (I8) {
                    if (r < wnb) acc = lm_mfma(i8x8_to_f16(w[u].x, w[u].y), wimg[(size_t)r * 64], acc);
                } else {
                    if (r < wnb) acc = lm_mfma(w[u], wimg[(size_t)r * 64], acc);
                }
            }
        }
    };
    auto tile_end = [&](int k) {
        const int j = k / cpt, c = k - j * cpt;
        if (c == cpt - 1) {  // tile j complete in every wave (uniform branch)
            float* Pb = P + (j & 1) * (kBgWaves * 128);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += dpp_f<kDppRor8>(acc[r]);  // hi + lo columns (lane + 8)
            if ((lane & 8) == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Pb[wave * 128 + ((lane >> 4) * 4 + r) * 8 + (lane & 7)] = acc[r];
            }
            acc = lm_float4{0.0f, 0.0f, 0.0f, 0.0f};
            __syncthreads();
            if (wave == (j & (kBgWaves - 1))) {  // tile j's 16 wave partials, summed in wave order
                const int i = lane >> 3, b = lane & 7;
                float v0 = 0.0f, v1 = 0.0f;
#pragma unroll
                for (int w = 0; w < kBgWaves; ++w) {
                    v0 += Pb[w * 128 + i * 8 + b];
                    v1 += Pb[w * 128 + (i + 8) * 8 + b];
                }
                R[j * 128 + i * 8 + b] = v0;
                R[j * 128 + (i + 8) * 8 + b] = v1;
            }
        }
    };
    int k = 0;
    // The next step's loads go out as soon as the current step's MFMAs have read their registers, BEFORE
    // the tile-end workgroup barrier: two steps stay in flight through every tile boundary.
    for (; k + 2 < nsteps; k += 2) {
        mfma_step(k, wa, sa);
        load_step(k + 2, wa, sa);
        tile_end(k);
        mfma_step(k + 1, wb, sb_);
        load_step(k + 3, wb, sb_);
        tile_end(k + 1);
    }
    if (k < nsteps) {
        mfma_step(k, wa, sa);
        tile_end(k);
    }
    if (k + 1 < nsteps) {
        mfma_step(k + 1, wb, sb_);
        tile_end(k + 1);
    }
    __syncthreads();
    if constexpr (NORM) {  // per-sequence 1/rms from the waves' sums of squares, in wave order
        if (tid < B) {
            float t = 0.0f;
            for (int w = 0; w < kBgWaves; ++w) t += red[w * 8 + tid];
            const float tep = t / (float)K;         // rms_kernel.cpp:17
            const float rms = sqrtf(tep + in.eps);  // :18
            inv[tid] = 1.0f / rms;                  // :19
        }
        __syncthreads();
    }
    if (in.stamps && tid == 0) {
        unsigned long long* p = in.stamps + (size_t)blockIdx.x * 4;
        p[0] = t_entry;
        p[1] = t_staged;
        p[2] = __builtin_amdgcn_s_memrealtime();
    }

    // ---- 6. epilogue (one split) or publish + the group's last arriver merges in split order
    const int items = ntg * 64;  // (tile, row pair i < 8, sequence slot b < 8)
    if (S == 1) {
        for (int it = tid; it < items; it += kBgThreads) {
            const int j = it >> 6, i = (it >> 3) & 7, b = it & 7;
            const float iv = NORM ? inv[b] : 1.0f;
            if (b < B) epi.store(t0 + j, i, b, R[j * 128 + i * 8 + b] * iv, R[j * 128 + (i + 8) * 8 + b] * iv, keys);
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

// ---------------------------------------------------------------- epilogues
// Plain rows: tile t holds rows 16t .. 16t+15. y[b][row] = resid[b][row] + (sum * rscale[row]) * scale
// (matmul_kernel.cpp:26 fused with add_kernel.cpp:5-14).
struct BgEpiStore {
    float* y;
    const float* resid;
    const float* rscale;
    float scale;
    int nrows;
    int ld;  // per-sequence stride of y / resid
    __device__ int row(int t, int i) const { return min(t * 16 + i, nrows - 1); }
    // (prefetching the residuals measured slower: C4 wo 8.89 -> 9.21 us, profiles/r4_bg_epi_prefetch_ab.txt)
    __device__ void pre_a(int, int, int) {}
    __device__ void pre_b() {}
    __device__ void one(int row, int b, float v) const {
        if (row >= nrows) return;
        float a = rscale ? v * rscale[row] : v;
        a = a * scale;
        const size_t o = (size_t)b * ld + row;
        y[o] = resid ? resid[o] + a : a;
    }
    __device__ void store(int t, int i, int b, float v0, float v1, unsigned long long*) const {
        one(t * 16 + i, b, v0);
        one(t * 16 + i + 8, b, v1);
    }
    __device__ void finish(unsigned long long*, int, int) const {}
};

// Fused q/k/v + RoPE + K/V cache write (model.cpp:54-67) per sequence: tile rows i and i + 8 are the
// RoPE pair {d, d + hd/2} of one head (8 pairs per tile). Cache [B][hkv][T][hd] per layer; sequence b's
// position is pos_dev[b * pos_stride].
template <typename KT>
struct BgEpiQKV {
    float* q_out;  // [B][hq*hd]
    KT* kc;        // layer base
    KT* vc;
    const int32_t* pos_dev;
    int pos_stride;
    const float* sin_t;
    const float* cos_t;
    int hq, hkv, hd, T;
    int kv_seq = 1;  // 1: sequence b owns cache heads [b*hkv, (b+1)*hkv); 0: one cache shared by every lane
                     // (prefill lanes of one sequence at consecutive positions)
    int p_t = -1, p_i = 0, p_b = 0, p_pos = 0;  // the prefetched item: its position, then its RoPE row
    float p_sin = 0.0f, p_cos = 0.0f;
    const float* rscale = nullptr;  // int8: per-row weight scales [(hq + 2 hkv) hd], applied before the rotation
    __device__ void pre_a(int t0, int ntg, int B) {
        const int it = threadIdx.x;
        if (it >= ntg * 64 || (it & 7) >= B) return;
        p_t = t0 + (it >> 6);
        p_i = (it >> 3) & 7;
        p_b = it & 7;
        p_pos = pos_dev[(size_t)p_b * pos_stride];
    }
    __device__ void pre_b() {
        if (p_t < 0) return;
        const int half = hd >> 1;
        const int u = p_t * 8 + p_i;
        const int uh = u / half, d = u - uh * half;
        if (uh < hq + hkv) {
            p_sin = sin_t[p_pos * half + d];
            p_cos = cos_t[p_pos * half + d];
        }
    }
    __device__ int row(int t, int i) const {
        const int half = hd >> 1;
        const int u = t * 8 + (i & 7);
        const int uh = u / half, d = u - uh * half;
        return uh * hd + d + (i >= 8 ? half : 0);
    }
    __device__ void store(int t, int i, int b, float a0, float a1, unsigned long long*) const {
        const int half = hd >> 1;
        const int u = t * 8 + i;
        const int uh = u / half, d = u - uh * half;
        if (rscale) {
            a0 *= rscale[uh * hd + d];
            a1 *= rscale[uh * hd + d + half];
        }
        const bool pre = t == p_t && i == p_i && b == p_b;
        const int pos = pre ? p_pos : pos_dev[(size_t)b * pos_stride];
        if (uh < hq + hkv) {  // rope_kernel.cpp:30-38
            const float fci = pre ? p_sin : sin_t[pos * half + d], fcr = pre ? p_cos : cos_t[pos * half + d];
            const float r0 = a0 * fcr - a1 * fci;
            const float r1 = a1 * fcr + a0 * fci;
            if (uh < hq) {
                float* q = q_out + ((size_t)b * hq + uh) * hd;
                q[d] = r0;
                q[d + half] = r1;
            } else {
                KT* kp = kc + (((size_t)b * kv_seq * hkv + (uh - hq)) * T + pos) * hd;
                kp[d] = from_f32<KT>(r0);
                kp[d + half] = from_f32<KT>(r1);
            }
        } else {
            KT* vp = vc + (((size_t)b * kv_seq * hkv + (uh - hq - hkv)) * T + pos) * hd;
            vp[d] = from_f32<KT>(a0);
            vp[d + half] = from_f32<KT>(a1);
        }
    }
    __device__ void finish(unsigned long long*, int, int) const {}
};

// Fused gate/up + activation (model.cpp:99-115): fused rows [gate(I); up(I)]; tile rows i / i + 8 are
// gate u / up u for u = 8t + i.
struct BgEpiSwiGLU {
    float* act;  // [B][inter]
    int inter;
    int silu;
    const float* rscale = nullptr;  // int8: per-row weight scales [2 inter], applied before the activation
    __device__ int row(int t, int i) const { return t * 8 + (i & 7) + (i >= 8 ? inter : 0); }
    __device__ void pre_a(int, int, int) {}
    __device__ void pre_b() {}
    __device__ void store(int t, int i, int b, float g, float up, unsigned long long*) const {
        if (rscale) {
            g *= rscale[t * 8 + i];
            up *= rscale[inter + t * 8 + i];
        }
        float sg = 1.0f / (1.0f + expf(-g));  // swiglu_kernel.cpp:12
        if (silu) sg = g * sg;
        act[(size_t)b * inter + t * 8 + i] = sg * up;  // :13
    }
    __device__ void finish(unsigned long long*, int, int) const {}
};

// LM head (model.cpp:136-139) per sequence + the first stage of the device argmax: the workgroup that
// ran a group's stores writes each sequence's max orderable key to keys_out[b][group].
struct BgEpiLogits {
    float* logits;                 // [B][ld]
    unsigned long long* keys_out;  // [B][key_ld]
    int nrows, ld, vocab_off, key_ld;
    const float* rscale = nullptr;  // int8: the row scales of this rank's rows of the table [nrows]
    __device__ int row(int t, int i) const { return min(t * 16 + i, nrows - 1); }
    __device__ void pre_a(int, int, int) {}
    __device__ void pre_b() {}
    __device__ void one(int row, int b, float v, unsigned long long* kl) const {
        if (row >= nrows) return;
        if (rscale) v *= rscale[row];  // the argmax key is taken after the scale
        logits[(size_t)b * ld + row] = v;
        atomicMax(kl + b, argmax_key(v, (unsigned)(row + vocab_off)));  // a max: order-independent
    }
    __device__ void store(int t, int i, int b, float v0, float v1, unsigned long long* kl) const {
        one(t * 16 + i, b, v0, kl);
        one(t * 16 + i + 8, b, v1, kl);
    }
    __device__ void finish(unsigned long long* kl, int g, int B) const {
        __syncthreads();
        if ((int)threadIdx.x < B) keys_out[(size_t)threadIdx.x * key_ld + g] = kl[threadIdx.x];
    }
};

// Row-major W [rows][K] -> the fragment layout of BgIn::tiled, rows in the epilogue's tile order (Epi::row:
// RoPE pairs, gate/up pairs, the last tile's clamped rows): out[(t * K/32 + kb) * 64 + l] (16-byte pieces) =
// W[row(t, l & 15)][32 kb + 8 (l >> 4) .. + 7]; int8: the same pieces at 8 bytes each, mxfp4: at 4 bytes each
// (BgIn::tiled). Init-time only (weights placed or replaced).
template <class Epi, typename WT>
__global__ void __launch_bounds__(256) bg_tile_kernel(const WT* __restrict__ W, int K, int ntiles, Epi epi,
                                                       void* __restrict__ out_) {
    constexpr size_t LB = bg_lane_bytes<WT>();
    using PV = typename std::conditional<LB == 4, unsigned, typename std::conditional<LB == 8, uint2, uint4>::type>::type;
    PV* out = reinterpret_cast<PV*>(out_);  // a lane's 8 weights
    const int nkb = K / 32;
    const size_t n = (size_t)ntiles * nkb * 64;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(p & 63);
        const size_t tb = p >> 6;
        const int t = (int)(tb / nkb), kb = (int)(tb - (size_t)t * nkb);
        const int row = epi.row(t, l & 15);
        out[p] = *reinterpret_cast<const PV*>(reinterpret_cast<const char*>(W) +
                                              ((size_t)row * nkb + (size_t)kb) * (4 * LB) + LB * (l >> 4));
    }
}
// mxfp4: the scale image of BgIn::tiled, out[(t * K/32 + kb) * 16 + i] = scales[row(t, i)][kb]
template <class Epi>
__global__ void __launch_bounds__(256) bg_tile_scales_kernel(const uint8_t* __restrict__ scales, int K, int ntiles, Epi epi,
                                                              uint8_t* __restrict__ out) {
    const int nkb = K / 32;
    const size_t n = (size_t)ntiles * nkb * 16;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(p & 15);
        const size_t tb = p >> 4;
        const int t = (int)(tb / nkb), kb = (int)(tb - (size_t)t * nkb);
        out[p] = scales[(size_t)epi.row(t, i) * nkb + kb];
    }
}

// mxfp4: `scales` (public layout) and `sout` (the scale image) are laid out beside the data
template <class Epi, typename WT>
hipError_t launch_bg_tile(const WT* W, int K, int ntiles, const Epi& epi, void* out, hipStream_t s,
                          const uint8_t* scales = nullptr, void* sout = nullptr) {
    if (K % 32) return hipErrorInvalidValue;
    const size_t n = (size_t)ntiles * (K / 32) * 64;
    const int blocks = (int)std::min<size_t>(8192, (n + 255) / 256);
    hipLaunchKernelGGL((bg_tile_kernel<Epi, WT>), dim3(blocks), dim3(256), 0, s, W, K, ntiles, epi, out);
    if constexpr (is_mx<WT>::value) {
        if (!scales || !sout) return hipErrorInvalidValue;
        const int sblocks = (int)std::min<size_t>(8192, (n / 4 + 255) / 256);
        hipLaunchKernelGGL((bg_tile_scales_kernel<Epi>), dim3(sblocks), dim3(256), 0, s, scales, K, ntiles, epi,
                           (uint8_t*)sout);
    }
    return hipGetLastError();
}
// bytes of a tiled matrix of `esize`-byte weights (2: fp16, 1: int8)
inline size_t bg_tiled_bytes(int ntiles, int K, int esize = 2) {
    return (size_t)ntiles * (size_t)(K / 32) * 512 * (size_t)esize;
}
// mxfp4: bytes of the data image (256 per block) and of the scale image (16 per block) of a tiled matrix
inline size_t bg_tiled_mx_bytes(int ntiles, int K) { return (size_t)ntiles * (size_t)(K / 32) * 256; }
inline size_t bg_tiled_mx_scale_bytes(int ntiles, int K) { return (size_t)ntiles * (size_t)(K / 32) * 16; }

// Allow the kernel its full dynamic LDS (once per instantiation; call outside stream capture).
template <class Epi, bool NORM, typename WT = __half>
hipError_t bg_allow_lds() {
    static const hipError_t e = [] {
        const hipError_t e4 = hipFuncSetAttribute(reinterpret_cast<const void*>(&bgemm_kernel<Epi, NORM, 4, WT>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, kBgLdsMax);
        const hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void*>(&bgemm_kernel<Epi, NORM, 2, WT>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, kBgLdsMax);
        if constexpr (!NORM) {  // (no 7-wide NORM kernel is ever launched: bg_launch_width)
            const hipError_t e7 = hipFuncSetAttribute(reinterpret_cast<const void*>(&bgemm_kernel<Epi, NORM, 7, WT>),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, kBgLdsMax);
            if (e7 != hipSuccess) return e7;
        }
        return e4 != hipSuccess ? e4 : e2;
    }();
    return e;
}

template <class Epi, typename WT>
hipError_t launch_bgemm(const WT* W, const BgIn& in_, const Epi& epi, const BgPlan& p, hipStream_t s) {
    BgIn in = in_;
    in.ntiles = p.ntiles;
    in.tpw = p.tpw;
    in.splits = p.splits;
    const dim3 grid(p.groups * p.splits);
    if (in.norm_w && p.splits != 1) return hipErrorInvalidValue;  // the fused RMS runs on one split only
    const int width = bg_launch_width(in.norm_w != nullptr, p.tpw, p.splits, in.K);
    if (in.norm_w && width == 2)
        hipLaunchKernelGGL((bgemm_kernel<Epi, true, 2, WT>), grid, dim3(kBgThreads), p.lds, s, W, in, epi);
    else if (in.norm_w)
        hipLaunchKernelGGL((bgemm_kernel<Epi, true, 4, WT>), grid, dim3(kBgThreads), p.lds, s, W, in, epi);
    else if (width == 2)
        hipLaunchKernelGGL((bgemm_kernel<Epi, false, 2, WT>), grid, dim3(kBgThreads), p.lds, s, W, in, epi);
    else if (width == 7)
        hipLaunchKernelGGL((bgemm_kernel<Epi, false, 7, WT>), grid, dim3(kBgThreads), p.lds, s, W, in, epi);
    else
        hipLaunchKernelGGL((bgemm_kernel<Epi, false, 4, WT>), grid, dim3(kBgThreads), p.lds, s, W, in, epi);
    return hipGetLastError();
}

}  // namespace sli
