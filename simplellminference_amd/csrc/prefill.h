// prefill.h — prompt prefill as real GEMMs over the prompt (the reference teacher-forces the
// prompt one token per forward, source/model/model.cpp:157-165, so every weight is streamed once per prompt
// token). Here a chunk of up to kPfMaxChunk prompt positions runs through each layer together:
//
//   1. pf_norm_split_kernel: per position RMSNorm (rms_kernel.cpp:5-23, fp32) and the split of the fp32
//      result into fp16 hi + lo (hi = fp16(h), lo = fp16(h - hi): h to ~2^-22 relative);
//   2. pgemm_kernel: Y[pos][row] = sum_k W[row][k] * H[pos][k] on MFMA (v_mfma_f32_16x16x32_f16), A = a 16-row
//      weight tile, B = 16 positions' hi columns, then the same tile with the lo columns into the same fp32
//      accumulator (W * (hi + lo)); a workgroup owns 16 AT WR weight rows x BM positions (PgCfg), so a weight row
//      is read from HBM once per BM positions (the decode step reads it once per position). Operands are staged
//      through an S-deep LDS ring by LDS-DMA (global_load_lds_dwordx4: one 1-KiB fragment image per
//      wave-instruction, read back conflict-free by ds_read_b128), S - 1 stages in flight behind a counted
//      vmcnt and a raw s_barrier (cdna_hip_programming.md §5 "Pipelining across barriers"), or the weight images
//      in a deeper ring of their own (PgCfg::SA, round 6); the fragment reads of
//      the next k-block are issued ahead of the current k-block's MFMAs (two register sets, across the stage
//      barrier too: PgCfg::PIPE, round 6, 5-20 % faster per GEMM, bit-identical sums). Fused epilogues:
//      RoPE + K/V cache rows + q (model.cpp:52-67), residual add (:86-90, :124-128), SwiGLU (:111-115,
//      written straight as the down projection's hi/lo operand);
//   3. pf_attn_mfma_kernel (fp16 KV, the default, or an FP8 E4M3 cache): block-causal attention of 16 chunk rows x
//      one head against
//      the cache rows 0 .. position (mha_kernel.cpp:36-77 per query: s_t = q.k_t * scale, softmax, sum p_t v_t):
//      S = K q^T on MFMA with q split hi/lo, online softmax in fp32, P V on MFMA with V read transposed
//      (ds_read_b64_tr_b16; FP8: ds_read_b64_tr_b8, codes widened to fp16 in registers) from LDS-DMA'd K/V tiles;
//      pf_attn_kernel, the VALU form (fp32, 64-position query
//      blocks, K/V tiles of 64 positions in LDS), serves fp32 KV caches.
// One pgemm_kernel body serves fp16, int8 and MXFP4 weights; a format struct (PgF16, PgI8, PgMx) holds what the
// weight type changes. int8 and MXFP4: stages of 128 k; a depth that is 64 mod 128 (e.g. Llama-2-7B int8 down at
// TP 4, 2752) ends with a half stage. MXFP4: the ring carries a scale image per stage too, and the block scale is
// applied to each k-block's tile in fp32 (PgMx).
// Which prompt position a chunk row is stands in device memory (PfSegs, the group table: 16-row groups, each a run of
// one sequence's positions), so one captured graph per chunk size serves every chunk of every prompt. A batch-1
// prompt's chunk is the table of one sequence at consecutive positions; a batched model's packed chunk
// (sli_model_prefill_seqs) carries groups of several sequences. The kernels that know a row's position (embedding,
// q/k/v epilogue, chunk attention) read the table; everything else sees independent chunk rows.
#pragma once
#include <type_traits>

#include "attn_mfma_f8.h"
#include "common.h"
#include "lds_mfma.h"
#include "mxfp4.h"

namespace sli {

constexpr int kPfMaxChunk = 256;  // prompt positions per weight pass

// The row map of a chunk: chunk rows 16 g .. 16 g + 15 are positions p0[g] .. p0[g] + 15 of sequence seq[g], the first
// nv[g] of them valid (the rest is padding: computed, never written to the cache); nv[g] == 0 is a padding group,
// which writes nothing to the cache and skips its attention. The engine's plans keep p0 % 16 == 0, so a row has the
// same 15 group-mates, and so the same attention tiles, however its sequence is packed; the one exception
// is the first group of a sequence continued from a start position (pf_pack_from), which runs from the start to the
// next 16-boundary: its rows only gain key tiles that are masked for them. The kernels themselves take any p0.
constexpr int kPfGroups = kPfMaxChunk / 16;
struct PfSegs {
    int32_t seq[kPfGroups], p0[kPfGroups], nv[kPfGroups];
};

// where chunk row m's token lies in the prompt buffer ([sequence][pld]); a group's padding rows repeat its last valid
// token, a padding group its first
__device__ __forceinline__ int pf_tok(const PfSegs* ps, int m, int pld) {
    const int g = m >> 4;
    return ps->seq[g] * pld + ps->p0[g] + min(m & 15, max(ps->nv[g] - 1, 0));
}

// ---------------------------------------------------------------- 1. embedding + RMSNorm / split
// x[m] = emb[token of chunk row m] (emb_kernel.cpp:4-21; pf_tok: row m's token comes from its sequence's prompt row,
// pld ids apart). emb_s: the int8 table's fp32 row scales (nullable), or the MXFP4 table's block scale bytes (mxfp4.h
// layout: a table decode per element)
template <typename WT>
__global__ void __launch_bounds__(256) pf_embed_kernel(const PfSegs* __restrict__ ps, const int32_t* __restrict__ prompt,
                                                      const WT* __restrict__ emb, const void* __restrict__ emb_s,
                                                      float* __restrict__ x, int D, int pld) {
    const int m = blockIdx.x;
    const int tok = prompt[pf_tok(ps, m, pld)];
    if constexpr (is_mx<WT>::value) {
        const uint8_t *data = reinterpret_cast<const uint8_t*>(emb), *sc = static_cast<const uint8_t*>(emb_s);
        for (int i = threadIdx.x; i < D; i += 256) x[(size_t)m * D + i] = mx_element(data, sc, (size_t)tok, D, i);
    } else {
        const float s = emb_s ? static_cast<const float*>(emb_s)[tok] : 1.0f;
        for (int i = threadIdx.x; i < D; i += 256) x[(size_t)m * D + i] = to_f32(emb[(size_t)tok * D + i]) * s;
    }
}

// one workgroup per chunk row: h = (x * 1/rms) * w (rms_kernel.cpp:12-22) or plain x (w == nullptr), as hi/lo.
// The row is held in registers (a float4 per thread and pass; D % 4 == 0, D <= 8192): one read of x, 8-byte
// hi / lo stores.
__global__ void __launch_bounds__(256) pf_norm_split_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           __half* __restrict__ hi, __half* __restrict__ lo, int D,
                                                           float eps) {
    constexpr int MAXV = 8;  // float4 per thread: D <= 8192
    const int m = blockIdx.x;
    const float* xr = x + (size_t)m * D;
    const int n4 = D / 4;
    float4 v[MAXV], wv[MAXV];
    float ss = 0.0f;
    // the norm weights are loaded with x (round 6: not after the reduction, one memory round trip fewer)
    const float4* w4 = reinterpret_cast<const float4*>(w ? w : xr);
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
        if (j * 256 + (int)threadIdx.x < n4) {
            v[j] = reinterpret_cast<const float4*>(xr)[j * 256 + threadIdx.x];
            wv[j] = w4[j * 256 + threadIdx.x];
            ss += v[j].x * v[j].x + v[j].y * v[j].y + v[j].z * v[j].z + v[j].w * v[j].w;
        }
    float inv = 1.0f;
    if (w) {
        ss = wave_sum(ss);
        __shared__ float red[4];
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
        __syncthreads();
        const float t = red[0] + red[1] + red[2] + red[3];
        const float tep = t / (float)D;      // rms_kernel.cpp:17
        const float rms = sqrtf(tep + eps);  // :18
        inv = 1.0f / rms;                    // :19
    }
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
        if (j * 256 + (int)threadIdx.x < n4) {
            const int i = (j * 256 + threadIdx.x) * 4;
            const float f[4] = {v[j].x, v[j].y, v[j].z, v[j].w}, g[4] = {wv[j].x, wv[j].y, wv[j].z, wv[j].w};
            __half hh[4], hl[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) pf_split(w ? (f[e] * inv) * g[e] : f[e], hh[e], hl[e]);  // :20-22
            *reinterpret_cast<uint2*>(hi + (size_t)m * D + i) = *reinterpret_cast<const uint2*>(hh);
            *reinterpret_cast<uint2*>(lo + (size_t)m * D + i) = *reinterpret_cast<const uint2*>(hl);
        }
}

// ---------------------------------------------------------------- 2. the GEMM
// The operand images travel by LDS-DMA (lds_mfma.h lm_dma: 1-KiB pieces, counted by the kernel's own vmcnt waits).
template <typename WT>
struct PgIn {
    const WT* W;        // [N][K] fp16 or int8 (row-major, PyTorch [out][in]; int8 row scales in the epilogue), or
                        // mxfp4 data [N][K / 2]
    const __half* Bhi;  // [M][K] activations, fp16 hi
    const __half* Blo;  // [M][K] fp16 lo
    int N, K, M;        // rows, depth, chunk rows (a multiple of BM)
    const uint8_t* Ws;  // mxfp4: e8m0 block scales [N][K / 32]; null otherwise
};

// Tiling: a workgroup of 2 WR waves owns BN = 16 AT WR weight rows x BM chunk rows; wave w holds the AT x BM/32
// accumulator tiles of rows 16 AT (w % WR) .. and position half w / WR. A stage covers KS depth: 64 for fp16
// weights, 128 for int8, so a weight row's slice is one whole 128-byte line (a chunk row's fp16 hi / lo slice
// one or two lines). Each LDS-DMA wave-instruction moves 1 KiB of whole lines (8 rows x 128 B or 4 x 256 B;
// fragment-shaped pieces of 16 rows x 64 B fetched every line twice and capped the ingest at ~29 GB/s per
// CU, tools/pgemm_lab); the 16-byte chunks of a row are XOR-swizzled by the row so the fragment reads
// (16 rows x 16 B per lane group) stay conflict-free. S stages in the LDS ring, S - 1 of them in flight.
// Epilogue contract: row(t, i) = weight row of 16-row tile t's row i (i < 16, always valid); store(t, i0, m, v)
// gets the fp32 sums of tile rows i0 .. i0+3 (i0 % 4 == 0) for chunk row m.
// AT_: 16-row weight tiles per wave (2: a wave's 32 rows; 4: 64 rows, so every B fragment read from LDS feeds twice
// the MFMAs). PIPE_: the fragment reads of k-block j + 1 issued before the MFMAs of k-block j (two register sets),
// across the stage barrier too, and every hi MFMA of a k-block ahead of its lo MFMAs (no back-to-back MFMAs on one
// accumulator); each tile's sums are added in the same order either way (bit-identical).
// SA_ > 0 (PIPE only): the weight (A) images get a ring of their own, SA_ stages deep (SA_ - 1 issued ahead), and
// the activation (B) images a 2-stage ring (one ahead): the A bytes come from HBM (read once per chunk), the B bytes
// from L2, so only A needs the deep prefetch, and B, the larger image, does not pay for it in LDS.
template <int BM_, int WR_, int S_, int AT_ = 2, bool PIPE_ = false, int SA_ = 0>
struct PgCfg {
    static constexpr int BM = BM_, WR = WR_, S = S_, AT = AT_, SA = SA_;
    static constexpr bool PIPE = PIPE_;
};

// 16-byte chunk swizzle of an image row (conflict-free fragment reads): rows of 128 B pair up in one 256-B
// bank span, so the chunk index is XORed with row / 2; rows of 256 B with the row
__host__ __device__ constexpr int pg_swz(int row, int row_bytes) { return row_bytes == 128 ? (row >> 1) & 7 : row & 15; }
// chunk swizzle of an mxfp4 weight image row (64 B): a k-block's fragment read is 16 rows x 16 B, 4 B per lane
__host__ __device__ constexpr int pg_mx_swz(int row, int row_bytes) { return row_bytes == 64 ? (row >> 2) & 3 : (row >> 1) & 7; }

// ---- weight formats (in the manner of attn_mfma.h AmF16 / AmF8): what the weight type changes, and nothing else.
// KS: depth per stage; A_ROW: weight row bytes per stage; CPK: 16-byte chunks of a weight row per 32-k block; swz: the
// weight image's chunk swizzle; SC_IMG: scale-image bytes per 16-row tile and stage; a_off / FRAG / a_frag: where in
// an image row (sw = swz(row)) lane group kg's 8 k of k-block kb lie, how many bytes, and their decode to 8 fp16;
// SCALED: a k-block's tile is summed on its own and scaled per row.
struct PgF16 {
    static constexpr int KS = 64, A_ROW = 128, CPK = 4, SC_IMG = 0, FRAG = 16;
    static constexpr bool SCALED = false;
    __host__ __device__ static constexpr int swz(int row) { return pg_swz(row, A_ROW); }
    __host__ __device__ static constexpr int a_off(int kb, int kg, int sw) { return ((4 * kb + kg) ^ sw) * 16; }
    __device__ __forceinline__ static u32x4 a_frag(const char* p) { return *reinterpret_cast<const u32x4*>(p); }
};
// int8: a depth that is 64 mod 128 ends with a half stage. k 32 kb + 8 kg .. +8: chunk 2 kb + kg / 2, half kg % 2;
// 8 int8 -> 8 fp16 exactly (common.h i8x8_to_f16)
struct PgI8 {
    static constexpr int KS = 128, A_ROW = 128, CPK = 2, SC_IMG = 0, FRAG = 8;
    static constexpr bool SCALED = false;
    __host__ __device__ static constexpr int swz(int row) { return pg_swz(row, A_ROW); }
    __host__ __device__ static constexpr int a_off(int kb, int kg, int sw) {
        return ((2 * kb + (kg >> 1)) ^ sw) * 16 + 8 * (kg & 1);
    }
    __device__ __forceinline__ static u32x4 a_frag(const char* p) {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
        return i8x8_to_f16(w.x, w.y);
    }
};
// MXFP4 (mxfp4.h: data [N][K/2], e8m0 scales [N][K/32]): a weight row's 128-k slice is half a line (64 B, one 1-KiB
// piece = one 16-row image), a chunk row's hi / lo slice two lines, the int8 geometry, so BM = 128 still fits two
// stages. (256-k stages tied or lost in every cell and could not take the fastest tilings:
// profiles/mxfp4_pgemm_lab.txt.)
// Scale scheme: one MFMA k-block is one MX block, so a (weight row, k-block) has one scale 2^e. The e2m1 codes are
// decoded to fp16 exactly and UNSCALED (a byte LUT through v_perm: the fp16 of every e2m1 magnitude has a zero low
// byte); the hi and lo MFMAs of a k-block run into a zeroed tile and acc = fma(tile, 2^e_row, acc) per C-fragment row
// in fp32, where every e8m0 byte 1 .. 254 is a normal number: no fp16 overflow or flush at any block exponent.
// The scale bytes travel through the ring too: global_load_lds_ubyte, a byte per lane into a dword of the stage's
// scale image [k-block][tile row], so a lane's four C rows of a tile are one ds_read_b128 and 2^e is dword << 23.
// Every wave issues the same number of pieces per stage (A, B and scale pieces), all LDS-DMA, all counted by
// pg_wait_stages; the kernel has no plain global load between its first DMA and its last wait.
// k 32 kb + 8 kg .. +8 of a row: chunk kb, bytes 4 kg .. +4.
struct PgMx {
    static constexpr int KS = 128, A_ROW = 64, CPK = 1, SC_IMG = 16 * (KS / 32) * 4, FRAG = 4;
    static constexpr bool SCALED = true;
    __host__ __device__ static constexpr int swz(int row) { return pg_mx_swz(row, A_ROW); }
    __host__ __device__ static constexpr int a_off(int kb, int kg, int sw) { return (kb ^ sw) * 16 + 4 * kg; }
    __device__ __forceinline__ static u32x4 a_frag(const char* p) {
        return pg_fp4_to_f16(*reinterpret_cast<const unsigned*>(p));
    }
};
template <typename WT>
using PgFmt = std::conditional_t<is_mx<WT>::value, PgMx, std::conditional_t<sizeof(WT) == 1, PgI8, PgF16>>;

// A stage image is [NA weight images][PT x (hi, lo) activation images][scale image], moved as pieces d = 0 .. NP - 1
// in that order: 1 KiB each, a scale piece 64 dwords. Wave w issues DPW of them per stage: pieces w DPW .. of the
// stage, or, with split rings and with a scaled format, its DPA weight pieces, then its DPB activation pieces, then
// its DPS scale pieces (piece()), so that a piece's kind is known from its place in the wave's list.
template <class Cfg, typename WT>
struct PgGeo {
    using F = PgFmt<WT>;
    static constexpr int BM = Cfg::BM, WR = Cfg::WR, S = Cfg::S, AT = Cfg::AT;
    static constexpr int WAVES = 2 * WR, THREADS = 64 * WAVES, BN = 16 * AT * WR;
    static constexpr int KS = F::KS;     // depth per stage
    static constexpr int KBS = KS / 32;  // MFMA k-blocks per stage
    static constexpr int A_ROW = F::A_ROW, B_ROW = KS * 2;  // 64 or 128 B; 128 or 256 B
    static constexpr int A_IMG = 16 * A_ROW, B_IMG = 16 * B_ROW;
    static constexpr int PT = BM / 16;  // position tiles per workgroup
    static constexpr int WPT = PT / 2;  // per wave
    static constexpr int NA = AT * WR;  // weight row tiles
    static constexpr int A_BYTES = NA * A_IMG, B_BYTES = 2 * PT * B_IMG;
    static constexpr int SC_BYTES = NA * F::SC_IMG;  // a dword per (k-block, tile row)
    static constexpr int STAGE = A_BYTES + B_BYTES + SC_BYTES;
    static constexpr int NPA = A_BYTES / 1024, NPB = B_BYTES / 1024, NPS = SC_BYTES / 256, NP = NPA + NPB + NPS;
    static constexpr int DPW = NP / WAVES;  // LDS-DMA instructions per wave and stage
    static constexpr int SA = Cfg::SA;      // split rings (PgCfg)
    static constexpr bool BY_KIND = SA > 0 || F::SCALED;
    static constexpr int DPA = BY_KIND ? NPA / WAVES : 0, DPB = BY_KIND ? NPB / WAVES : 0, DPS = BY_KIND ? NPS / WAVES : 0;
    static constexpr size_t LDS = SA ? (size_t)SA * A_BYTES + (size_t)S * B_BYTES : (size_t)S * STAGE;
    // piece j of wave w's list, and a piece's byte offset in the stage image
    __host__ __device__ static constexpr int piece(int w, int j) {
        if (!BY_KIND) return w * DPW + j;
        return j < DPA ? w * DPA + j : j < DPA + DPB ? NPA + w * DPB + j - DPA : NPA + NPB + w * DPS + j - DPA - DPB;
    }
    __host__ __device__ static constexpr int dst(int d) {
        return (!F::SCALED || d < NPA + NPB) ? d * 1024 : A_BYTES + B_BYTES + (d - NPA - NPB) * 256;
    }
    static_assert(A_ROW == 16 * F::CPK * KBS && 1024 % A_ROW == 0 && WPT >= 1 && (AT == 2 || AT == 4), "tiling");
    static_assert(NP % WAVES == 0 && (!BY_KIND || (NPA % WAVES == 0 && NPB % WAVES == 0 && NPS % WAVES == 0)), "pieces");
    static_assert(S >= 2 && S <= 8 && (S - 1) * DPW <= 63, "ring depth (vmcnt counts 63 loads)");
    // (SA > S: A(s) must be issued in an earlier iteration than B(s), the wait below counts on it; SA == S computed
    // wrong sums in tools/pgemm_lab). A scaled format has one ring.
    static_assert(SA == 0 || (!F::SCALED && Cfg::PIPE && S == 2 && SA > S && (SA - 1) * DPA + DPB <= 63), "split rings");
    static_assert(LDS <= 160 * 1024, "LDS");
};

// Where piece d of a stage comes from: lane `lane` lands at byte 16 lane (scale piece: dword `lane`) of the piece, i.e.
// image row lane / cpr, physical chunk lane % cpr (cpr = 16-B chunks per image row), so it loads the row's logical
// chunk c = (lane % cpr) ^ swizzle(row); a scale piece's lane loads the byte of (k-block, tile row) = its dword.
// The source is byte off + s adv of the row's K-slice at stage s. The last stage may be short: vkb < KBS valid
// k-blocks. There a logical chunk c steps back to c mod (valid chunks) (`back` bytes; a weight k-block is CPK chunks,
// an activation one 4, a scale one a byte): a reload of a valid part of the stage, in bounds and never read. Shared
// with the host (tests/cpp/pgemm_pieces.cpp enumerates every piece of every table tiling).
struct PgPiece {
    int kind;  // 0: weights, 1: hi, 2: lo activations, 3: weight scales
    int row;   // row of the block: weight row 16 tile + r of the row block, or chunk row of the position block
    int off;   // byte of the row's stage-0 slice
    int adv;   // bytes per stage
    int back;  // bytes to step back in a short last stage
    __host__ __device__ constexpr long at(int s, bool tail) const { return off + (long)s * adv - (tail ? back : 0); }
};
template <class Geo>
__host__ __device__ constexpr PgPiece pg_piece(int d, int lane, int vkb) {
    using F = typename Geo::F;
    if (d < Geo::NPA) {
        constexpr int cpr = Geo::A_ROW / 16;
        const int o = d * 1024;
        const int r = (o % Geo::A_IMG) / Geo::A_ROW + lane / cpr;
        const int c = (lane % cpr) ^ F::swz(r);
        return {0, o / Geo::A_IMG * 16 + r, c * 16, Geo::A_ROW, (c - c % (F::CPK * vkb)) * 16};
    } else if (!F::SCALED || d < Geo::NPA + Geo::NPB) {
        constexpr int cpr = Geo::B_ROW / 16;
        const int o = (d - Geo::NPA) * 1024;
        const int u = o / Geo::B_IMG;  // image 2 pt + (lo ? 1 : 0)
        const int r = (o % Geo::B_IMG) / Geo::B_ROW + lane / cpr;
        const int c = (lane % cpr) ^ pg_swz(r, Geo::B_ROW);
        return {1 + (u & 1), (u >> 1) * 16 + r, c * 16, Geo::B_ROW, (c - c % (4 * vkb)) * 16};
    } else {  // dword q of the scale image [k-block][tile row]
        const int q = (d - Geo::NPA - Geo::NPB) * 64 + lane;
        const int kb = q / (Geo::NA * 16);
        return {3, q - kb * (Geo::NA * 16), kb, Geo::KBS, kb - kb % vkb};
    }
}

// wait until at most `later` stages of DPW images each are still in flight (later: 0 .. 6)
template <int DPW>
__device__ __forceinline__ void pg_wait_stages(int later) {
    switch (later) {
        case 0: lm_wait_vm<0>(); break;
        case 1: lm_wait_vm<1 * DPW>(); break;
        case 2: lm_wait_vm<(2 * DPW > 63 ? 63 : 2 * DPW)>(); break;
        case 3: lm_wait_vm<(3 * DPW > 63 ? 63 : 3 * DPW)>(); break;
        case 4: lm_wait_vm<(4 * DPW > 63 ? 63 : 4 * DPW)>(); break;
        case 5: lm_wait_vm<(5 * DPW > 63 ? 63 : 5 * DPW)>(); break;
        default: lm_wait_vm<(6 * DPW > 63 ? 63 : 6 * DPW)>(); break;
    }
}

template <class Epi, class Cfg, typename WT>
__global__ void __launch_bounds__(128 * Cfg::WR) pgemm_kernel(PgIn<WT> in, Epi epi) {
    using Geo = PgGeo<Cfg, WT>;
    using F = typename Geo::F;
    constexpr int KBS = Geo::KBS, BM = Geo::BM, WR = Geo::WR, S = Geo::S, AT = Geo::AT, NA = Geo::NA, WPT = Geo::WPT;
    constexpr int DPW = Geo::DPW, DPA = Geo::DPA, DPB = Geo::DPB;
    extern __shared__ __attribute__((aligned(1024))) char pg_smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __builtin_assume(wave >= 0 && wave < Geo::WAVES);
    const int wr = wave % WR, wp = wave / WR;  // row pair, position half
    const int PB = in.M / BM;
    // workgroups that share a row block run on one XCD (blocks b and b + 8 share one under round-robin
    // placement; speed only): the second read of the weight rows hits that XCD's L2
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int rb = (slot / PB) * 8 + xcd, pb = slot - (slot / PB) * PB;
    const int nrb = (in.N + Geo::BN - 1) / Geo::BN;
    if (rb >= nrb) return;  // (uniform) padding of the grid to a multiple of 8 row blocks
    // stages: the last one may be short, kt / 32 valid k-blocks: its pieces step back (pg_piece), and only its valid
    // k-blocks are multiplied. K is a multiple of 64 (the callers' check), so a short 128-k stage holds KBS / 2; the
    // pipelined loop, which multiplies k-blocks in pairs, is told so and tests once per pair.
    const int ns = (in.K + Geo::KS - 1) / Geo::KS;
    const int kt = in.K % Geo::KS;  // depth of a short last stage (0: none)
    const bool half_tail = kt != 0;
    const int vkb = half_tail ? (Cfg::PIPE ? KBS / 2 : kt / 32) : KBS;  // k-blocks of the last stage
    const int nt = in.N >> 4;                   // row tiles
    const unsigned ring = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)pg_smem;

    // this wave's pieces Geo::piece(wave, j): stage-0 source, bytes per stage, the short last stage's step back
    const char* src[DPW];
    int adv[DPW], back[DPW];
#pragma unroll
    for (int j = 0; j < DPW; ++j) {
        const PgPiece p = pg_piece<Geo>(Geo::piece(wave, j), lane, vkb);
        const char* rowp;
        if (p.kind == 0 || (F::SCALED && p.kind == 3)) {
            const int row = epi.row(min(rb * NA + (p.row >> 4), nt - 1), p.row & 15);
            if (F::SCALED && p.kind == 3)
                rowp = reinterpret_cast<const char*>(in.Ws) + (size_t)row * (in.K / kMxBlock);
            else
                rowp = reinterpret_cast<const char*>(in.W) + (size_t)row * wt_row_bytes<WT>(in.K);
        } else {
            const __half* B = p.kind == 2 ? in.Blo : in.Bhi;
            rowp = reinterpret_cast<const char*>(B) + (size_t)(pb * BM + p.row) * in.K * 2;
        }
        src[j] = rowp + p.off;
        adv[j] = p.adv;
        back[j] = p.back;
    }
    // pieces [j0, j1) of stage s; `slot`: the LDS address the stage image would start at
    auto issue_pieces = [&](int s, int j0, int j1, unsigned slot) {
        const bool tail = half_tail && s == ns - 1;
#pragma unroll
        for (int j = j0; j < j1; ++j) {
            const int d = Geo::piece(wave, j);
#ifdef PG_LAB_SKIP  // tools/pgemm_lab only (bit 0: no A pieces, bit 1: no B pieces): timing bounds, wrong sums
            if (((PG_LAB_SKIP & 1) && d < Geo::NPA) || ((PG_LAB_SKIP & 2) && d >= Geo::NPA && d < Geo::NPA + Geo::NPB))
                continue;
#endif
            // (one offset, then one add: subtracted from src on its own, the step-back is hoisted out of the stage loop
            // as a second pointer per piece, 2 VGPRs each)
            const char* g = src[j] + ((ptrdiff_t)s * adv[j] - (tail ? back[j] : 0));
            if (F::SCALED && j >= DPA + DPB)
                lm_dma_u8(g, slot + (unsigned)Geo::dst(d));
            else
                lm_dma(g, slot + (unsigned)Geo::dst(d));
        }
    };
    auto issue = [&](int s) { issue_pieces(s, 0, DPW, ring + (unsigned)((s % S) * Geo::STAGE)); };
    // split rings: A stage s in slot s % SA at ring, B stage s in slot s % 2 behind the A ring
    constexpr int SAD = Geo::SA ? Geo::SA : 1;
    auto issue_a = [&](int s) { issue_pieces(s, 0, DPA, ring + (unsigned)((s % SAD) * Geo::A_BYTES)); };
    auto issue_b = [&](int s) {
        issue_pieces(s, DPA, DPA + DPB, ring + (unsigned)((Geo::SA - 1) * Geo::A_BYTES + (s & 1) * Geo::B_BYTES));
    };
    lm_float4 acc[AT][WPT];
#pragma unroll
    for (int a = 0; a < AT; ++a)
#pragma unroll
        for (int b = 0; b < WPT; ++b) acc[a][b] = lm_float4{0.0f, 0.0f, 0.0f, 0.0f};

    // fragment read offsets: lane l reads row / column r = l & 15, k group kg = l >> 4 of each 32-k block
    const int kg = lane >> 4, r16 = lane & 15;
    const int sa = F::swz(r16), sb = pg_swz(r16, Geo::B_ROW);
    if constexpr (Geo::SA == 0) {
        for (int s = 0; s < S - 1 && s < ns; ++s) issue(s);
    } else {  // the schedule of iterations -(SA - 1) .. -1: B(i + 1), then A(i + SA - 1)
        for (int i = 1 - Geo::SA; i < 0; ++i) {
            if (i + 1 >= 0 && i + 1 < ns) issue_b(i + 1);
            if (i + Geo::SA - 1 >= 0 && i + Geo::SA - 1 < ns) issue_a(i + Geo::SA - 1);
        }
    }
    // the fragments of one k-block; sc (scaled formats): the scale dwords of this lane's C rows 4 kg .. +4 per tile
    struct Frags {
        u32x4 a[AT], h[WPT], l[WPT], sc[F::SCALED ? AT : 1];
    };
    // k-block kb of a stage buffer (A images at st; B images, then the scale image, at stb)
    auto read_frags = [&](const char* st, const char* stb, int kb, Frags& f) {
#pragma unroll
        for (int a = 0; a < AT; ++a) {
            const int ti = wr * AT + a;
            f.a[a] = F::a_frag(st + ti * Geo::A_IMG + r16 * Geo::A_ROW + F::a_off(kb, kg, sa));
            if constexpr (F::SCALED)
                f.sc[a] = *reinterpret_cast<const u32x4*>(stb + Geo::B_BYTES + ((kb * NA + ti) * 16 + 4 * kg) * 4);
        }
#pragma unroll
        for (int b = 0; b < WPT; ++b) {
            const int pt = wp * WPT + b;
            const char* img = stb + (2 * pt) * Geo::B_IMG + r16 * Geo::B_ROW + ((4 * kb + kg) ^ sb) * 16;
            f.h[b] = *reinterpret_cast<const u32x4*>(img);
            f.l[b] = *reinterpret_cast<const u32x4*>(img + Geo::B_IMG);
        }
    };
    // every hi MFMA of the k-block, then every lo one: into acc, or (scaled) into a zeroed tile that one fp32 fma
    // per C row adds to acc times 2^(byte - 127)
    auto mfmas = [&](const Frags& f) {
        lm_float4 tile[AT][WPT];
        lm_float4(&t)[AT][WPT] = *(F::SCALED ? &tile : &acc);
#if defined(PG_LAB_MFMA) && PG_LAB_MFMA == 0  // tools/pgemm_lab only: no MFMA (data movement alone)
#pragma unroll
        for (int b = 0; b < WPT; ++b)
#pragma unroll
            for (int a = 0; a < AT; ++a) {
                t[a][b] = F::SCALED ? lm_float4{0.0f, 0.0f, 0.0f, 0.0f} : acc[a][b];
                t[a][b][0] += __uint_as_float(f.a[a][0] ^ f.h[b][0] ^ f.l[b][0]);
            }
#else
#pragma unroll
        for (int b = 0; b < WPT; ++b)
#pragma unroll
            for (int a = 0; a < AT; ++a)
                t[a][b] = lm_mfma(f.a[a], f.h[b], F::SCALED ? lm_float4{0.0f, 0.0f, 0.0f, 0.0f} : acc[a][b]);
#if !(defined(PG_LAB_MFMA) && PG_LAB_MFMA == 1)  // PG_LAB_MFMA 1: the hi MFMA only
#pragma unroll
        for (int b = 0; b < WPT; ++b)
#pragma unroll
            for (int a = 0; a < AT; ++a) t[a][b] = lm_mfma(f.a[a], f.l[b], t[a][b]);
#endif
#endif
        if constexpr (F::SCALED) {
#pragma unroll
            for (int a = 0; a < AT; ++a) {
                float sc[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) sc[e] = __uint_as_float(f.sc[a][e] << 23);
#pragma unroll
                for (int b = 0; b < WPT; ++b)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[a][b][e] = fmaf(tile[a][b][e], sc[e], acc[a][b][e]);
            }
        }
    };
    // PIPE: set x holds even k-blocks, set y odd ones (KBS is even, and so is a short stage's KBS / 2 at 128-k
    // stages): per stage read(0) -> x, MFMA(y: the previous stage's last k-block), read(1) -> y, MFMA(x), ... The
    // stage barrier follows this wave's lgkmcnt(0), so the previous stage's buffer is free for the DMA issued after it
    // while its last fragments wait in registers.
    static_assert(!Cfg::PIPE || (KBS % 2 == 0 && (KBS / 2 % 2 == 0 || Geo::KS == 64)), "k-blocks per stage");
    Frags x, y;
    for (int s = 0; s < ns; ++s) {
        const char *st, *stb;
        if constexpr (Geo::SA == 0) {
            // this wave's pieces of stage s landed: it issued whole stages only, DPW LDS-DMAs each and nothing else
            // that the counter counts, so at most min(S - 2, ns - 1 - s) later stages are behind them in order
            pg_wait_stages<DPW>(min(S - 2, ns - 1 - s));
            if constexpr (Cfg::PIPE) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();  // every wave's pieces of s landed; every wave is done with s - 1
            if (s + S - 1 < ns) issue(s + S - 1);  // into the buffer of s - 1
            st = pg_smem + (size_t)(s % S) * Geo::STAGE;
            stb = st + Geo::A_BYTES;
        } else {
            // B(s) was the first load of iteration s - 1; only that iteration's A pieces (if it issued any) were
            // issued after it, and A(s) before it
            if (s + Geo::SA - 2 < ns)
                lm_wait_vm<DPA>();
            else
                lm_wait_vm<0>();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (s + 1 < ns) issue_b(s + 1);
            if (s + Geo::SA - 1 < ns) issue_a(s + Geo::SA - 1);
            st = pg_smem + (size_t)(s % SAD) * Geo::A_BYTES;
            stb = pg_smem + (size_t)Geo::SA * Geo::A_BYTES + (size_t)(s & 1) * Geo::B_BYTES;
        }
        const int kbs = s == ns - 1 ? vkb : KBS;  // wave-uniform
        if constexpr (Cfg::PIPE) {
#pragma unroll
            for (int kb = 0; kb < KBS; kb += 2) {
                if (kb >= kbs) break;
                read_frags(st, stb, kb, x);
                if (s > 0 || kb > 0) mfmas(y);
                read_frags(st, stb, kb + 1, y);
                mfmas(x);
            }
        } else {
#pragma unroll
            for (int kb = 0; kb < KBS; ++kb) {
                if (kb >= kbs) break;
                read_frags(st, stb, kb, x);
                mfmas(x);
            }
        }
    }
    if constexpr (Cfg::PIPE) mfmas(y);
    // C[i][n] of a 16x16 tile: lane l holds rows 4 (l >> 4) + r, column l & 15
    const int i0 = 4 * (lane >> 4);
#pragma unroll
    for (int a = 0; a < AT; ++a) {
        const int t = rb * NA + wr * AT + a;
        if (t >= nt) continue;
#pragma unroll
        for (int b = 0; b < WPT; ++b) {
            const int m = pb * BM + (wp * WPT + b) * 16 + r16;
            const float v[4] = {acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]};
            epi.store(t, i0, m, v);
        }
    }
}

// ---- epilogues. Tiles hold 4-row groups {first(u), first(u + 1), second(u), second(u + 1)} where a pair is a
// RoPE pair {d, d + hd/2} (q/k/v) or {gate u, up u}, so each lane's 4 rows are 2 complete pairs.
template <typename KT>
struct PgEpiQKV {  // model.cpp:52-67: q (fp32 [M][hq*hd]), rotated k / v rows of the cache at the row's position (KT:
                   // float, __half, or f8e4m3: codes). Chunk row m = 16 g + r is position p0[g] + r of sequence seq[g],
                   // written for r < nv[g].
    float* q;
    KT* kc;  // this layer's cache of every sequence [B][hkv][T][hd] (a batch-1 model: B = 1)
    KT* vc;
    const float* rscale;  // int8 row scales (nullable)
    const float* sin_t;
    const float* cos_t;
    int hq, hkv, hd, T;
    const PfSegs* segs;
    __device__ int row(int t, int i) const {
        const int half = hd >> 1;
        const int u = t * 8 + (i >> 2) * 2 + (i & 1);
        const int uh = u / half, d = u - uh * half;
        return uh * hd + d + ((i & 2) ? half : 0);
    }
    __device__ void store(int t, int i0, int m, const float* v) const {
        // A wave's rows of one call are one group (pgemm_kernel: m = 16 * position tile + lane % 16), and nothing writes
        // the table while a kernel runs. Said outright (the uniform index, the constant address space) the three reads
        // are scalar loads that need not wait behind the stores of the call before; left to the compiler they were
        // vector loads, one dependent round trip per call.
        const int g = __builtin_amdgcn_readfirstlane(m >> 4), r = m & 15;
        const auto* tb = (const __attribute__((address_space(4))) PfSegs*)segs;
        store_at(t, i0, m, v, tb->p0[g] + r, r < tb->nv[g], (size_t)tb->seq[g] * hkv * T * hd);
    }
    // pos: chunk row m's position; valid: its K / V rows are written (where pos < T); kv0: its sequence's offset in
    // kc / vc (elements)
    __device__ void store_at(int t, int i0, int m, const float* v, int pos, bool valid, size_t kv0) const {
        // units u, u + 1 (u even): d, d + 1 of one head (hd / 2 is even), so every store is a pair
        const int half = hd >> 1;
        const int u = t * 8 + (i0 >> 2) * 2;
        const int uh = u / half, d = u - uh * half;
        float a0[2] = {v[0], v[1]}, a1[2] = {v[2], v[3]};  // first / second element of the pairs of u, u + 1
        if (rscale) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                a0[e] *= rscale[uh * hd + d + e];
                a1[e] *= rscale[uh * hd + d + e + half];
            }
        }
        if (uh < hq + hkv) {  // rope_kernel.cpp:30-38
            const int pp = min(pos, T - 1);
            float r0[2], r1[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float fci = sin_t[pp * half + d + e], fcr = cos_t[pp * half + d + e];
                r0[e] = a0[e] * fcr - a1[e] * fci;
                r1[e] = a1[e] * fcr + a0[e] * fci;
            }
            if (uh < hq) {
                float* qr = q + (size_t)m * hq * hd + (size_t)uh * hd;
                *reinterpret_cast<float2*>(qr + d) = make_float2(r0[0], r0[1]);
                *reinterpret_cast<float2*>(qr + d + half) = make_float2(r1[0], r1[1]);
            } else if (valid && pos < T) {
                KT* kr = kc + kv0 + ((size_t)(uh - hq) * T + pos) * hd;
                store2(kr + d, r0);
                store2(kr + d + half, r1);
            }
        } else if (valid && pos < T) {
            KT* vr = vc + kv0 + ((size_t)(uh - hq - hkv) * T + pos) * hd;
            store2(vr + d, a0);
            store2(vr + d + half, a1);
        }
    }
    __device__ static void store2(KT* p, const float* f) {
        if constexpr (sizeof(KT) == 1) {  // FP8 E4M3 codes through the one codec (common.h); d is even: aligned
            const unsigned c0 = from_f32<KT>(f[0]).bits, c1 = from_f32<KT>(f[1]).bits;
            *reinterpret_cast<unsigned short*>(p) = (unsigned short)(c0 | (c1 << 8));
        } else if constexpr (sizeof(KT) == 2) {
            __half h[2] = {__float2half_rn(f[0]), __float2half_rn(f[1])};
            *reinterpret_cast<unsigned*>(p) = *reinterpret_cast<const unsigned*>(h);
        } else {
            *reinterpret_cast<float2*>(p) = make_float2(f[0], f[1]);
        }
    }
};

struct PgEpiSwiGLU {  // model.cpp:99-115: act = sigmoid(g) * u (or SiLU), stored as the down GEMM's hi / lo
    __half* ahi;
    __half* alo;
    const float* rscale;
    int inter, silu;
    __device__ int row(int t, int i) const { return t * 8 + (i >> 2) * 2 + (i & 1) + ((i & 2) ? inter : 0); }
    __device__ void store(int t, int i0, int m, const float* v) const {
        const int u = t * 8 + (i0 >> 2) * 2;  // units u, u + 1: one 4-byte hi and lo store each
        __half hh[2], hl[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float g = v[e], up = v[2 + e];
            if (rscale) {
                g *= rscale[u + e];
                up *= rscale[inter + u + e];
            }
            float sg = 1.0f / (1.0f + expf(-g));  // swiglu_kernel.cpp:12
            if (silu) sg = g * sg;
            pf_split(sg * up, hh[e], hl[e]);  // :13
        }
        *reinterpret_cast<unsigned*>(ahi + (size_t)m * inter + u) = *reinterpret_cast<const unsigned*>(hh);
        *reinterpret_cast<unsigned*>(alo + (size_t)m * inter + u) = *reinterpret_cast<const unsigned*>(hl);
    }
};

struct PgEpiResid {  // y[m][row] = resid[m][row] + sum * row scale (matmul_kernel.cpp:26 + add_kernel.cpp:5-14)
    float* y;        // [M][ld]: the residual stream (in place), or this rank's partial under TP
    const float* resid;  // the residual stream (tensor-parallel ranks > 0: null, their partial has none)
    const float* rscale;
    int nrows, ld;
    __device__ int row(int t, int i) const { return min(t * 16 + i, nrows - 1); }
    __device__ void store(int t, int i0, int m, const float* v) const {
        const int row = t * 16 + i0;  // rows row .. row + 3 (nrows % 16 == 0: the host's check)
        const size_t i = (size_t)m * ld + row;
        float4 p = make_float4(v[0], v[1], v[2], v[3]);
        if (rscale) {
            const float4 sc = *reinterpret_cast<const float4*>(rscale + row);
            p = make_float4(p.x * sc.x, p.y * sc.y, p.z * sc.z, p.w * sc.w);
        }
        if (resid) {
            const float4 r = *reinterpret_cast<const float4*>(resid + i);
            p = make_float4(r.x + p.x, r.y + p.y, r.z + p.z, r.w + p.w);
        }
        *reinterpret_cast<float4*>(y + i) = p;
    }
};

// The LM head over chunk rows (role 3, "logits"): y[m][row] = sum * row scale for row < nrows, and nothing else. nrows
// need not be a multiple of 16 (the small presets have a vocabulary of 1000): the launch's N is nrows rounded up to 16,
// the row map clamps the last tile's weight rows as PgEpiResid's does, and the store and the int8 row-scale load are
// masked at nrows, so columns nrows .. ld - 1 are never written. A full 4-row group is PgEpiResid's store without a
// residual, bit for bit.
struct PgEpiLogits {
    float* y;  // [M][ld], ld >= nrows, ld % 4 == 0
    const float* rscale;
    int nrows, ld;
    __device__ int row(int t, int i) const { return min(t * 16 + i, nrows - 1); }
    __device__ void store(int t, int i0, int m, const float* v) const {
        const int row = t * 16 + i0;
        const size_t i = (size_t)m * ld + row;
        if (row + 3 < nrows) {
            float4 p = make_float4(v[0], v[1], v[2], v[3]);
            if (rscale) {
                const float4 sc = *reinterpret_cast<const float4*>(rscale + row);
                p = make_float4(p.x * sc.x, p.y * sc.y, p.z * sc.z, p.w * sc.w);
            }
            *reinterpret_cast<float4*>(y + i) = p;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (row + e < nrows) y[i + e] = rscale ? v[e] * rscale[row + e] : v[e];
        }
    }
};
// the N a role-3 launch is given for nrows weight rows
constexpr int pg_logits_n(int nrows) { return (nrows + 15) & ~15; }

template <class Epi, class Cfg, typename WT>
hipError_t launch_pgemm(const PgIn<WT>& in, const Epi& epi, hipStream_t s) {
    using Geo = PgGeo<Cfg, WT>;
    const int nrb = (in.N + Geo::BN - 1) / Geo::BN;
    const int nrb8 = (nrb + 7) / 8 * 8;
    const dim3 grid(nrb8 * (in.M / Geo::BM));
    hipLaunchKernelGGL((pgemm_kernel<Epi, Cfg, WT>), grid, dim3(Geo::THREADS), Geo::LDS, s, in, epi);
    return hipGetLastError();
}

template <class Epi, class Cfg, typename WT>
hipError_t pgemm_allow_lds() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&pgemm_kernel<Epi, Cfg, WT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)PgGeo<Cfg, WT>::LDS);
}

// The GEMM tiling (PgCfg<BM, WR, S, AT, PIPE, SA>) per weight type, projection role and chunk size: the fastest of
// the tools/pgemm_lab sweeps on the 7B shapes (profiles/r3_pgemm_lab.txt; round 6: the pipelined fragment reads,
// 5-20 % faster at every tiling, the M = 128 choices, profiles/r6b_pg_pipe.txt, and the M = 256 ones re-timed with
// the weights streamed from HBM as in the engine, profiles/r6b_pg_cold.txt).
// role 0: qkv, 1: gate/up, 2: wo / down (N = D: few row blocks, so small chunk blocks for a full grid), 3: logits
// (N = V: many row blocks, as gate/up, whose cells it starts on; nobody has timed them at N = V yet).
// f(PgCfg<...>{}) is called with the chosen tiling. The one table: the engine's launches, its LDS opt-in and the
// kernel-level entry point (sli_prefill_gemm) all pick through it.
template <typename WT, class F>
int pg_pick(int M, int role, F&& f) {
    if (role == 3) role = 1;
    if constexpr (is_mx<WT>::value) {
        // the fastest of tools/pgemm_lab's LAB_MX sweep per 7B shape and chunk size, weights rotated over four copies
        // (profiles/mxfp4_pgemm_lab.txt; PIPE is not yet measured for this format, SA is refused for it). wo / down
        // (N = D, few row blocks) want 32-row chunk blocks.
        if (M == 32) return f(PgCfg<32, 2, 4, 2>{});
        if (role == 2) return M == 256 ? f(PgCfg<32, 4, 4, 2>{}) : f(PgCfg<32, 2, 4, 2>{});
        if (role == 1) return M == 128 ? f(PgCfg<128, 4, 2, 2>{}) : f(PgCfg<64, 4, 3, 2>{});
        if (M == 256) return f(PgCfg<128, 4, 2, 2>{});
        return M == 128 ? f(PgCfg<64, 4, 3, 2>{}) : f(PgCfg<32, 4, 4, 2>{});
    } else if constexpr (std::is_same<WT, int8_t>::value) {
        if (M == 32) return f(PgCfg<32, 2, 4, 2, true>{});
        if (role == 2) return M == 256 ? f(PgCfg<64, 2, 2, 2, true>{}) : f(PgCfg<32, 2, 4, 2, true>{});
        if (role == 1) return M == 128 ? f(PgCfg<128, 4, 2, 2, true>{}) : f(PgCfg<64, 4, 2, 2, true>{});
        return M == 256 ? f(PgCfg<128, 4, 2, 2, true>{}) : f(PgCfg<64, 4, 2, 2, true>{});
    } else {
        if (M == 32) return f(PgCfg<32, 2, 4, 2, true>{});
        if (role == 2) return M == 256 ? f(PgCfg<64, 2, 3, 2, true>{}) : f(PgCfg<32, 2, 4, 2, true>{});
        if (M == 64 || (M == 128 && role == 0)) return f(PgCfg<64, 2, 3, 2, true>{});
        // M = 256 with the weights streamed from HBM (profiles/r6b_pg_cold.txt): 8-wave workgroups
        // (q/k/v: the weights in a 4-deep ring of their own, profiles/r6b_pg_split.txt)
        if (M == 256) return role == 0 ? f(PgCfg<128, 4, 2, 2, true, 4>{}) : f(PgCfg<64, 4, 3, 2, true>{});
        return f(PgCfg<128, 2, 2, 2, true>{});
    }
}

constexpr int kPfSizes[4] = {32, 64, 128, 256};  // prefill chunk sizes, the rows of the table (the last is kPfMaxChunk)

// the LDS opt-in of every tiling the table can pick for this epilogue and weight type
template <class Epi, typename WT>
hipError_t pg_allow_lds_all() {
    hipError_t err = hipSuccess;
    for (int M : kPfSizes)
        for (int role = 0; role < 4; ++role)
            pg_pick<WT>(M, role, [&](auto cfg) {
                if (err == hipSuccess) err = pgemm_allow_lds<Epi, decltype(cfg), WT>();
                return 0;
            });
    return err;
}

// ---------------------------------------------------------------- 3. block-causal attention
// grid (M / 64, hq); 4 waves x 16 queries; lane l: query l & 15 of the wave, dims [c * HD/4, (c+1) * HD/4) with
// c = l >> 4. Scores: the 4 lanes of a query add their quarter dot products (xor 16 / 32 exchanges); every lane
// of a query keeps the same online-softmax state (m, l) and its quarter of o. Output attn / l as hi / lo.
// A one-sequence kernel. Contract: the four groups of a 64-row block are consecutive positions of sequence 0, so the
// block reads its start position from its first group, p0[4 * blockIdx.x], and never reads seq or nv. Every table
// built for one sequence satisfies it (a padding group is computed like any other row; nothing reads its result).
constexpr int kPaQB = 64;  // queries per workgroup
constexpr int kPaKT = 64;  // keys per LDS tile

template <typename KT>
struct PfAttnArgs {
    const float* q;    // [M][hq*hd]
    const KT* kc;      // layer base [hkv][T][hd]
    const KT* vc;
    __half* ohi;       // [M][hq*hd]
    __half* olo;
    int hq, hkv, T;
    float scale;       // 1/sqrt(hd) (mha_kernel.cpp:41)
};

template <typename KT, int HD>
__global__ void __launch_bounds__(256) pf_attn_kernel(PfAttnArgs<KT> a, const PfSegs* __restrict__ ps) {
    constexpr int QD = HD / 4;  // dims per lane
    __shared__ __attribute__((aligned(16))) KT ks[kPaKT][HD];
    __shared__ __attribute__((aligned(16))) KT vs[kPaKT][HD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.y, G = a.hq / a.hkv, kvh = h / G;
    const int p0 = ps->p0[(kPaQB / 16) * blockIdx.x];             // position of the block's row 0
    const int mb = wave * 16 + (lane & 15);                       // this lane's row of the block
    const int mi = blockIdx.x * kPaQB + mb;                       // its query (chunk row)
    const int c = lane >> 4;
    const int pos = p0 + mb;                                      // its position
    const int pos_max = p0 + kPaQB - 1;                           // the block's last query position
    const int nt = min(pos_max, a.T - 1) / kPaKT + 1;             // key tiles
    float qv[QD], o[QD];
#pragma unroll
    for (int e = 0; e < QD; ++e) {
        qv[e] = a.q[(size_t)mi * a.hq * HD + (size_t)h * HD + c * QD + e];
        o[e] = 0.0f;
    }
    float mx = -INFINITY, l = 0.0f;
    const KT* kb = a.kc + (size_t)kvh * a.T * HD;
    const KT* vb = a.vc + (size_t)kvh * a.T * HD;
    constexpr int V16 = 16 / (int)sizeof(KT);  // elements per 16-byte vector
    for (int tt = 0; tt < nt; ++tt) {
        const int t0 = tt * kPaKT;
        __syncthreads();
        for (int i = threadIdx.x; i < kPaKT * HD / V16; i += 256) {  // the tile's K and V rows
            const int r = i / (HD / V16), cc = i - r * (HD / V16);
            const int t = min(t0 + r, a.T - 1);
            reinterpret_cast<u32x4*>(&ks[r][0])[cc] = reinterpret_cast<const u32x4*>(kb + (size_t)t * HD)[cc];
            reinterpret_cast<u32x4*>(&vs[r][0])[cc] = reinterpret_cast<const u32x4*>(vb + (size_t)t * HD)[cc];
        }
        __syncthreads();
        float s[kPaKT];
        float tmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < kPaKT; ++j) {
            float d = 0.0f;
#pragma unroll
            for (int e = 0; e < QD; ++e) d = fmaf(qv[e], to_f32(ks[j][c * QD + e]), d);
            d = sum_xor16(d);
            d = sum_xor32(d);
            s[j] = (t0 + j <= pos) ? d * a.scale : -INFINITY;  // mha_kernel.cpp:51-60 (sum * scale), causal
            tmax = fmaxf(tmax, s[j]);
        }
        const float mn = fmaxf(mx, tmax);
        const float corr = mn == -INFINITY ? 1.0f : expf(mx - mn);
        l *= corr;
#pragma unroll
        for (int e = 0; e < QD; ++e) o[e] *= corr;
        mx = mn;
#pragma unroll
        for (int j = 0; j < kPaKT; ++j) {
            const float p = (t0 + j <= pos) ? expf(s[j] - mx) : 0.0f;
            l += p;
#pragma unroll
            for (int e = 0; e < QD; ++e) o[e] = fmaf(p, to_f32(vs[j][c * QD + e]), o[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < QD; ++e) {
        const size_t idx = (size_t)mi * a.hq * HD + (size_t)h * HD + c * QD + e;
        pf_split(o[e] / l, a.ohi[idx], a.olo[idx]);
    }
}

// ---- 3b. block-causal attention on MFMA (fp16 or FP8 E4M3 cache). A workgroup = 16 chunk rows (queries) of one
// head; its 4 waves split the key range into 32-key tiles (wave w takes tiles w, w + 4, ...) and merge their
// (max, sum, o) through LDS at the end. Per tile a wave:
//   - LDS-DMAs K and V rows t0 .. t0+31 (1-KiB pieces) into its own images, 16-B chunks XOR-swizzled;
//   - Sᵀ = K Qᵀ: C[key][query] on v_mfma_f32_16x16x32_f16, A = K rows (exact fp16), B = Qᵀ as hi + lo fp16
//     (two MFMAs into one accumulator);
//   - online softmax per query (a lane's 8 keys, then the 4 lane groups of a query by xor 16 / 32);
//   - Oᵀ += Vᵀ Pᵀ: B = Pᵀ straight from the Sᵀ accumulators (lane l holds query l & 15 and 8 keys of the tile,
//     in the k order of the B operand), P as hi + lo; A = Vᵀ by transposed LDS reads whose row blocks are
//     exactly those keys.
// One body serves both cache formats, as the decode attention's does (attn_mfma.h am_attn): the format struct F
// (AmF16, AmF8) holds what a cache row's bytes change, i.e. the element size, the chunk swizzles, which key of the
// tile A row i of S MFMA kt is (fp16: 16 kt + i; FP8: 8 (i >> 2) + 4 kt + (i & 3)) and so which key a lane's S
// accumulator holds (fp16: 16 kt + 4 g + r; FP8: 8 g + 4 kt + r), the K fragment read (FP8: 8 codes widened
// exactly to fp16 in registers) and the Vᵀ reads (fp16: two ds_read_b64_tr_b16 per 16-d tile, FP8: one
// ds_read_b64_tr_b8). After the widening the arithmetic is the fp16 cache's.
// mha_kernel.cpp:36-77 per query: s_t = (q . k_t) * scale, softmax over t <= position, o = sum p_t v_t.
template <class F, int HD>
struct PaGeo {
    static constexpr int ROWB = HD * F::EB;      // bytes per image row
    static constexpr int IMG = 32 * ROWB;        // one 32-key image
    static constexpr int WAVE = 2 * IMG;         // K + V
    static constexpr int PIECES = WAVE / 1024;   // DMA instructions per tile
    static constexpr int CPR = ROWB / 16;        // 16-B chunks per row
    static constexpr int NT = HD / 16;           // 16-d tiles (O)
    // the end-of-kernel merge reuses the tile LDS as [4 waves][NT][64 lanes][4] floats + (m, l) [4][64] each: 34 KiB
    // (hd 128) or 18 KiB (hd 64), more than the four FP8 tile images (32 / 16 KiB)
    static constexpr int MERGE = (4 * NT * 64 * 4 + 2 * 4 * 64) * 4;
    static constexpr int LDS = 4 * WAVE > MERGE ? 4 * WAVE : MERGE;
    static_assert(HD == 64 || HD == 128, "head_dim");
    static_assert(PIECES >= 2 && PIECES % 2 == 0 && 1024 % ROWB == 0, "whole 1-KiB pieces per K and per V image");
};

// Workgroup x is group x of the table; kc / vc hold every sequence's rows ([B][hkv][T][hd]) and a padding group leaves
// at once, as a whole.
template <class F, int HD>
__global__ void __launch_bounds__(256) pf_attn_mfma_kernel(PfAttnArgs<typename F::KT> a, const PfSegs* __restrict__ ps) {
    using G = PaGeo<F, HD>;
    using KT = typename F::KT;
    constexpr int ND = HD / 32, NT = G::NT;  // 32-d blocks (S), 16-d tiles (O)
    __shared__ __attribute__((aligned(1024))) char sm[G::LDS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = lane >> 4, i16 = lane & 15;
    const int h = blockIdx.y, kvh = h / (a.hq / a.hkv);
    const int gseq = ps->seq[blockIdx.x], gp0 = ps->p0[blockIdx.x];
    // (uniform: one table entry per workgroup; ahead of every barrier and DMA)
    if (ps->nv[blockIdx.x] == 0) return;
    const int mq = blockIdx.x * 16 + i16;  // this lane's query (chunk row)
    const int pos = gp0 + i16;
    const int last = min(gp0 + 15, a.T - 1);  // the group's last query position
    const int ntiles = last / 32 + 1;
    const size_t qs = (size_t)a.hq * HD;
    // Qᵀ as the B operand: lane l = query l & 15, d = 32 db + 8 g .. +8, fp32 -> hi + lo
    u32x4 qh[ND], ql[ND];
#pragma unroll
    for (int db = 0; db < ND; ++db) {
        const float4* qp = reinterpret_cast<const float4*>(a.q + (size_t)mq * qs + (size_t)h * HD + db * 32 + g * 8);
        const float4 v0 = qp[0], v1 = qp[1];
        const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        __half hh[8], hl[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) pf_split(f[e], hh[e], hl[e]);
        qh[db] = *reinterpret_cast<const u32x4*>(hh);
        ql[db] = *reinterpret_cast<const u32x4*>(hl);
    }
    lm_float4 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) o[t] = lm_float4{0.0f, 0.0f, 0.0f, 0.0f};
    float mx = -INFINITY, l = 0.0f;
    char* kimg = sm + wave * G::WAVE;
    const unsigned kbase = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)kimg;
    const unsigned vbase = kbase + G::IMG;
    const KT* kc = a.kc + ((size_t)gseq * a.hkv + kvh) * a.T * HD;
    const KT* vc = a.vc + ((size_t)gseq * a.hkv + kvh) * a.T * HD;
    for (int tt = wave; tt < ntiles; tt += 4) {
        const int t0 = tt * 32;
        // K pieces 0 .. P/2-1, V pieces P/2 .. P-1; lane i of a piece: row (piece rows) + i / CPR, physical
        // chunk i % CPR <- logical chunk (i % CPR) ^ swizzle(row)
#pragma unroll
        for (int j = 0; j < G::PIECES; ++j) {
            const bool isv = j >= G::PIECES / 2;
            const int jj = isv ? j - G::PIECES / 2 : j;
            const int r = jj * (1024 / G::ROWB) + lane / G::CPR;
            const int c = (lane % G::CPR) ^ (isv ? F::swz_v(r, G::ROWB) : F::swz_k(r, G::ROWB));
            const KT* src = (isv ? vc : kc) + (size_t)min(t0 + r, a.T - 1) * HD + c * (16 / F::EB);
            lm_dma(src, (isv ? vbase : kbase) + (unsigned)(jj * 1024));
        }
        lm_wait_vm<0>();
        // Sᵀ[key][query]: A row i16 of MFMA kt is key t0 + F::a_row(kt, i16)
        lm_float4 sacc[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            sacc[kt] = lm_float4{0.0f, 0.0f, 0.0f, 0.0f};
            const int r = F::a_row(kt, i16);
            const char* krow = kimg + r * G::ROWB;
            const int sw = F::swz_k(r, G::ROWB);
#pragma unroll
            for (int db = 0; db < ND; ++db) {
                const u32x4 kf = F::k_frag(krow, sw, db, g);
                sacc[kt] = lm_mfma(kf, qh[db], sacc[kt]);
                sacc[kt] = lm_mfma(kf, ql[db], sacc[kt]);
            }
        }
        // lane holds keys F::acc_key(t0, g, kt, r) of query mq
        float sv[8];
        float cmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = F::acc_key(t0, g, kt, r);
                const float v = key <= pos ? sacc[kt][r] * a.scale : -INFINITY;
                sv[kt * 4 + r] = v;
                cmax = fmaxf(cmax, v);
            }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
        const float mn = fmaxf(mx, cmax);
        const float corr = mn == -INFINITY ? 1.0f : expf(mx - mn);
        float pv[8], psum = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            pv[e] = sv[e] == -INFINITY ? 0.0f : expf(sv[e] - mn);
            psum += pv[e];
        }
        psum += __shfl_xor(psum, 16);
        psum += __shfl_xor(psum, 32);
        l = l * corr + psum;
        mx = mn;
        __half ph[8], pl[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) pf_split(pv[e], ph[e], pl[e]);
        const u32x4 pfh = *reinterpret_cast<const u32x4*>(ph);
        const u32x4 pfl = *reinterpret_cast<const u32x4*>(pl);
        // the Vᵀ operand's transposed reads: the keys of a lane group's row block are the keys of its P elements
        uint2 x[NT * F::VR];
        F::template v_read<NT, G::ROWB>(vbase, lane, x);
        lm_tr_landed(x);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            o[t] *= corr;
            const u32x4 vf = F::v_frag(x, t);
            o[t] = lm_mfma(vf, pfh, o[t]);
            o[t] = lm_mfma(vf, pfl, o[t]);
        }
    }
    // merge the 4 key splits: wave w publishes (mx, l, o) and merges 16-d tiles t = w, w + 4, ...
    __syncthreads();
    float* fo = reinterpret_cast<float*>(sm);                         // [wave][NT][64 lanes][4]
    float* fm = fo + 4 * NT * 64 * 4;                                 // [wave][64]
    float* fl = fm + 4 * 64;
#pragma unroll
    for (int t = 0; t < NT; ++t)
        *reinterpret_cast<lm_float4*>(fo + ((wave * NT + t) * 64 + lane) * 4) = o[t];
    fm[wave * 64 + lane] = mx;
    fl[wave * 64 + lane] = l;
    __syncthreads();
    float m4[4], w4[4], M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        m4[w] = fm[w * 64 + lane];
        M = fmaxf(M, m4[w]);
    }
    float L = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        w4[w] = m4[w] == -INFINITY ? 0.0f : expf(m4[w] - M);
        L += fl[w * 64 + lane] * w4[w];
    }
    const float inv = 1.0f / L;
    for (int t = wave; t < NT; t += 4) {
        lm_float4 acc = lm_float4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int w = 0; w < 4; ++w) acc += *reinterpret_cast<const lm_float4*>(fo + ((w * NT + t) * 64 + lane) * 4) * w4[w];
        // lane holds d = 16 t + 4 g + r of query mq
        const size_t idx = (size_t)mq * qs + (size_t)h * HD + t * 16 + 4 * g;
        __half hh[4], hl[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) pf_split(acc[r] * inv, hh[r], hl[r]);
        *reinterpret_cast<uint2*>(a.ohi + idx) = *reinterpret_cast<const uint2*>(hh);
        *reinterpret_cast<uint2*>(a.olo + idx) = *reinterpret_cast<const uint2*>(hl);
    }
}

// The attention of M chunk rows (hd 64 or 128: the caller's check): an fp16 or FP8 cache on MFMA, 16 chunk rows per
// workgroup; an fp32 cache on the VALU kernel, 64 chunk rows per workgroup, so at M = 32 it reads q and writes
// ohi / olo for rows 32 .. 63 too (the buffers hold at least 64 rows). The engine and sli_prefill_attn launch
// through here. The VALU kernel is a one-sequence kernel (its contract stands at pf_attn_kernel: the four groups of a
// 64-row block are consecutive positions of sequence 0); a packed table of several sequences takes the MFMA kernel
// alone, and the callers that build one refuse an fp32 cache first.
constexpr int pf_attn_rows(bool mfma_cache, int M) { return mfma_cache ? M : (M + kPaQB - 1) / kPaQB * kPaQB; }

template <typename KT>
hipError_t launch_pf_attn(const PfAttnArgs<KT>& aa, int hd, int M, const PfSegs* ps, hipStream_t s) {
    if constexpr (!std::is_same<KT, float>::value) {
        using F = std::conditional_t<std::is_same<KT, f8e4m3>::value, AmF8, AmF16>;
        const dim3 ag(M / 16, aa.hq);
        if (hd == 128)
            hipLaunchKernelGGL((pf_attn_mfma_kernel<F, 128>), ag, dim3(256), 0, s, aa, ps);
        else
            hipLaunchKernelGGL((pf_attn_mfma_kernel<F, 64>), ag, dim3(256), 0, s, aa, ps);
    } else {
        const dim3 ag((M + kPaQB - 1) / kPaQB, aa.hq);
        if (hd == 128)
            hipLaunchKernelGGL((pf_attn_kernel<KT, 128>), ag, dim3(256), 0, s, aa, ps);
        else
            hipLaunchKernelGGL((pf_attn_kernel<KT, 64>), ag, dim3(256), 0, s, aa, ps);
    }
    return hipGetLastError();
}

}  // namespace sli
