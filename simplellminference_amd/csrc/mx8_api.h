// mx8_api.h — what the engine launches of mx8.hip (the MXFP8 quantisers, the block-scaled MFMA prefill GEMM of
// pgemm_mx8.h and the block-scaled batched decode projection of bgemm_mx8.h): plain host functions, so that translation
// unit keeps the one compiled copy of those kernels. The host side of the batched projection (its launch arguments,
// its plan and the planner) lives here, where both translation units read it.
#pragma once
#include <algorithm>

#include "bgemm.h"
#include "common.h"

namespace sli {

// the LDS opt-in of every tiling of every epilogue; once, outside any stream capture
int mx8_prepare();
// codes [M][D], scales [M][D / 32] of RMSNorm(x row) * w (w null: of x), or of hi + lo
int mx8_norm_quant(const float* x, const float* w, void* codes, void* scales, int M, int D, float eps, hipStream_t s);
int mx8_pair_quant(const void* hi, const void* lo, void* codes, void* scales, int M, int D, hipStream_t s);
// one pgemm_mx8_kernel launch under the group table `segs` (read by role 0 alone); nothing is checked here
int mx8_gemm(const void* data, const void* scales, const void* acodes, const void* ascales, int N, int K, int M,
             const sli_pgemm_epilogue& e, const void* segs, sli_pgemm_tiling* tiling, hipStream_t s);

// ---------------------------------------------------------------- the batched decode projection (bgemm_mx8.h)
constexpr int kBg8Stage = 128;  // k of one MFMA issue: the unit of every k-range
constexpr int kBg8Ring = 4;     // 16-byte weight loads a wave keeps in flight

// A workgroup owns `tpw` consecutive 16-row tiles and one of `splits` ranges of 128-k stages; its 16 waves are wt tiles
// in flight x wk k-slices of the range (wt * wk == 16).
struct Bg8Plan {
    int ntiles = 0, tpw = 1, splits = 1, groups = 0, wt = 1, wk = 16;
    size_t lds = 0;
};

struct Bg8In {
    const float* x;       // [B][K] fp32 activations
    const float* norm_w;  // fused RMSNorm weight [K], or nullptr
    float eps;
    int K, B;
    int ntiles, tpw, splits, wt, wk;  // from the plan (launch_bgemm_mx8)
    float* ws;           // splits > 1: partials [ntiles][splits][16][8]
    unsigned* counters;  // splits > 1: [groups] arrival counters, zero between launches
    // tiled != 0: the images of bg8_tile_kernel. Data: (tile t, stage s) is one KiB at (t * K/128 + s) * 1024, lane l's 16
    // bytes (the codes of row(t, l % 16), k 128 s + 32 (l / 16) .. + 32) at l * 16. Scales: 64 B per (tile, stage), lane
    // l's byte at l. 0: the public layout, data [rows][K / 2] and scales [rows][K / 32].
    int tiled;
    const uint8_t* w;
    const uint8_t* wscale;
    unsigned long long* stamps = nullptr;  // diagnostic (tools/bgemm_mx8_lab): per-workgroup s_memrealtime x4
};

// dynamic LDS: bgemm.h's scratch, the code image (1 KiB per stage: 8 sequences x 128 B) and its scale image (32 B per
// stage), the waves' double-buffered partial tiles when k-slices are reduced, the finished tiles
inline size_t bg8_lds_bytes(int K, int splits, int tpw, int wk) {
    const int ns = K / kBg8Stage;
    const int nss = (ns + splits - 1) / splits;
    return (size_t)kBgScratch + (size_t)nss * (1024 + 32) + (wk > 1 ? (size_t)kBgPBytes : 0) + (size_t)tpw * 512;
}

inline bool bg8_pow2_waves(int wt, int wk) {
    return wt >= 1 && wk >= 1 && wt * wk == kBgWaves && (wt & (wt - 1)) == 0;
}

// What a forced plan must satisfy (the conditions the planner searches under), or the reason it does not
inline const char* bg8_plan_refusal(int ntiles, int K, bool norm, int tpw, int splits, int wt, int wk) {
    if (ntiles < 1 || K < kBg8Stage || K % kBg8Stage) return "K must be a positive multiple of 128";
    if (tpw < 1 || tpw > (1 << 16) || splits < 1) return "forced plan: tpw and splits must be >= 1";
    if (!bg8_pow2_waves(wt, wk)) return "forced plan: wt * wk must be 16 (powers of two)";
    if (norm && splits != 1) return "forced plan: the fused RMSNorm runs on one split";
    if (splits > K / kBg8Stage) return "forced plan: more splits than 128-k stages";
    if (bg8_lds_bytes(K, splits, tpw, wk) > (size_t)kBgLdsMax) return "forced plan: LDS image too large";
    return nullptr;
}

// The one place that decides (tpw, splits, wt, wk) of a launch. Cost in units of one stage of one wave (a 1-KiB weight
// load and its MFMA issue, about 0.45 us), its constants read off tools/bgemm_mx8_lab's sweep of forced plans on the five
// Llama-3-8B launches and its per-workgroup stamps (profiles/bgemm_mx8_lab.txt). A workgroup runs ceil(tpw / wt) rounds;
// a round costs the longest k-slice, ceil(stages / wk) stages, and with wk > 1 a workgroup barrier and a wk-way LDS
// reduce of the partial tiles (wk == 1: neither; the wave stores its tile itself). Staging and quantising is paid once
// per workgroup and is mostly a floor: 6.4 us for 1024 k, 8.0 us for 4096 k (13.5 units + 0.14 per stage), and every
// further 4096 k of a split is a serial load-and-quantise loop of its own (10 units; down on one split lost by 2x). A
// split adds the write-through hand-off (wo: 2.4 us from first entry to last end, plus the last arriver's merge). The
// grid runs in ceil(workgroups / cus) passes.
// max_groups > 0: no more workgroup groups than that (the LM head writes one argmax key per group into a fixed row).
inline Bg8Plan bg_mx8_plan(int ntiles, int K, int B, bool norm, int cus = 256, int max_groups = 0) {
    Bg8Plan best;
    if (ntiles < 1 || K < kBg8Stage || K % kBg8Stage || B < 1 || B > kBgMaxBatch) return best;
    const int ns = K / kBg8Stage;
    double best_cost = 1e30;
    for (int s = 1; s <= 16 && s <= ns; ++s) {
        if (norm && s > 1) break;  // the rms needs the whole row
        const int nss = (ns + s - 1) / s;
        for (int wk = 1; wk <= kBgWaves; wk *= 2) {
            const int wt = kBgWaves / wk;
            const int cps = (nss + wk - 1) / wk;
            for (int tpw = 1; tpw <= 64; ++tpw) {
                if (bg8_lds_bytes(K, s, tpw, wk) > (size_t)kBgLdsMax) break;
                const int groups = (ntiles + tpw - 1) / tpw;
                if (max_groups > 0 && groups > max_groups) continue;
                const int rounds = (tpw + wt - 1) / wt;
                const int passes = (groups * s + cus - 1) / cus;
                // a stage costs a wave its share of the CU's HBM bandwidth once most waves stream, else the load latency
                // over the ring: waves without a tile (wt > tpw) stream nothing, and nothing speeds up for it
                const int active = wk * std::min(wt, tpw);
                const double stage = std::max(1.0, active / 12.0);
                double per_wg = rounds * (cps * stage + 1.0 + (wk > 1 ? 1.0 + 0.1 * wk : 0.0));
                per_wg += 3.0 + (13.5 + 0.14 * nss + 10.0 * ((nss + 31) / 32 - 1)) * (0.5 + 0.5 * B / 8.0);  // entry, epilogue; staging
                if (s > 1) per_wg += 14.0 + 0.25 * s * tpw;
                const double cost = passes * per_wg;
                if (cost < best_cost - 1e-9) {
                    best_cost = cost;
                    best.ntiles = ntiles;
                    best.tpw = tpw;
                    best.splits = s;
                    best.groups = groups;
                    best.wt = wt;
                    best.wk = wk;
                    best.lds = bg8_lds_bytes(K, s, tpw, wk);
                }
                if (groups == 1) break;
            }
        }
    }
    return best;
}

// device workspace of a plan: split partials (256-B aligned), then one arrival counter per group (bgemm.h's layout)
inline size_t bg8_part_bytes(const Bg8Plan& p) {
    return p.splits > 1 ? (((size_t)p.ntiles * p.splits * 128 * sizeof(float) + 255) & ~(size_t)255) : 0;
}
inline size_t bg8_ws_bytes(const Bg8Plan& p) { return bg8_part_bytes(p) + sizeof(unsigned) * (size_t)p.groups + 256; }

// the LDS opt-in of every instantiation; once, outside any stream capture
int mx8_bgemm_prepare();
// one bgemm_mx8_kernel launch; nothing is checked here
int mx8_bgemm(const Bg8In& in, const BgEpiQKV<float>& e, const Bg8Plan& p, hipStream_t s);
int mx8_bgemm(const Bg8In& in, const BgEpiQKV<__half>& e, const Bg8Plan& p, hipStream_t s);
int mx8_bgemm(const Bg8In& in, const BgEpiQKV<f8e4m3>& e, const Bg8Plan& p, hipStream_t s);
int mx8_bgemm(const Bg8In& in, const BgEpiStore& e, const Bg8Plan& p, hipStream_t s);
int mx8_bgemm(const Bg8In& in, const BgEpiSwiGLU& e, const Bg8Plan& p, hipStream_t s);
int mx8_bgemm(const Bg8In& in, const BgEpiLogits& e, const Bg8Plan& p, hipStream_t s);
// public-layout data / scales -> the images of Bg8In::tiled, rows in the epilogue's tile order (only row() is used)
int mx8_bg_tile(const void* data, const void* scales, int K, int ntiles, const BgEpiQKV<__half>& e, void* out, void* sout, hipStream_t s);
int mx8_bg_tile(const void* data, const void* scales, int K, int ntiles, const BgEpiStore& e, void* out, void* sout, hipStream_t s);
int mx8_bg_tile(const void* data, const void* scales, int K, int ntiles, const BgEpiSwiGLU& e, void* out, void* sout, hipStream_t s);
int mx8_bg_tile(const void* data, const void* scales, int K, int ntiles, const BgEpiLogits& e, void* out, void* sout, hipStream_t s);

// the checks sli_batch_gemm makes of an epilogue descriptor (bgemm_ops.h), shared with sli_batch_gemm_mx8
int bgo_check_epilogue(const std::string& fn, const sli_bgemm_epilogue& e, bool norm);
int64_t bgo_epilogue_rows(const sli_bgemm_epilogue& e);

}  // namespace sli
