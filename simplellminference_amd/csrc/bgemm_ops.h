// bgemm_ops.h — one batched decode projection as a kernel-level entry point (include/sli.h "batched decode stages,
// for tests and labs"): one bgemm_kernel launch (bgemm.h) on caller-provided device buffers, with the epilogue,
// weight type, layout and plan of any launch the engine's StepRecorder makes for batch > 1. Included once, at the
// end of engine.hip, and written over the engine's own template arguments (launch_bgemm<Epi, WT> and
// launch_bg_tile<Epi, WT> for exactly the (Epi, WT) pairs StepRecorder::b_* and bg_build_tiles name), so the library
// holds ONE compiled copy of every batched kernel and the entry launches the very code objects a model step
// launches; role and norm are paired as the engine pairs them, which keeps that set closed. A forced plan is
// checked on the host against everything bgemm_kernel assumes (the conditions bg_plan searches under); whatever
// the kernel would read or write out of bounds for is refused here, before anything touches the device.
// MXFP4 weights have entries of their own (sli_batch_gemm_mxfp4, sli_matmul_batch_mxfp4: the matrix is two arrays, data
// and block scales, and sli_batch_gemm keeps refusing the type); they share sli_batch_gemm's body (bgo_entry), so the
// contract is the same, and with tiled != 0 they build the data image and the scale image inside the workspace.
#pragma once
#include "bgemm.h"
#include "common.h"

namespace sli {

static bool bgo_al16(const void* p) { return (uintptr_t)p % 16 == 0; }

// Workspace: split partials, arrival counters (bg_ws_bytes), then for tiled = 1 the fragment-layout image of W at
// the next 256-byte boundary (the layout of sli_matmul_batch_i8's workspace).
static size_t bgo_image_off(const BgPlan& p) { return (bg_ws_bytes(p) + 255) & ~(size_t)255; }
static size_t bgo_ws_bytes(const BgPlan& p, int K, int esize, int tiled) {
    return tiled ? bgo_image_off(p) + bg_tiled_bytes(p.ntiles, K, esize) : bg_ws_bytes(p);
}
// mxfp4, tiled = 1: the data image at the same place, the scale image right behind it (a multiple of 256 bytes on)
static size_t bgo_ws_bytes_mx(const BgPlan& p, int K, int tiled) {
    return tiled ? bgo_image_off(p) + bg_tiled_mx_bytes(p.ntiles, K) + bg_tiled_mx_scale_bytes(p.ntiles, K) : bg_ws_bytes(p);
}

// The plan of a launch: io->tpw == 0 asks bg_plan (the engine's planner, the device's CU count); otherwise
// (io->tpw, io->splits) is forced after the checks below. Returns nullptr and fills p / io, or the refusal.
static const char* bgo_plan(int ntiles, int K, int B, bool norm, sli_bgemm_plan* io, BgPlan& p) {
    if (ntiles < 1 || K < 32 || K % 32 != 0 || K > (1 << 20)) return "K must be a positive multiple of 32";
    if (B < 1 || B > kBgMaxBatch) return "batch must be in [1, 8]";
    if ((int64_t)ntiles * K >= ((int64_t)1 << 36)) return "shape too large";
    const int nkb = K / 32;
    if (io->tpw == 0) {
        p = bg_plan(ntiles, K, B, norm, device_cus());
        if (p.groups <= 0) return "no plan fits (a fused norm stages the whole row: K <= 4096)";
    } else {
        const int tpw = io->tpw, s = io->splits;
        if (tpw < 1 || s < 1) return "forced plan: tpw and splits must be >= 1";
        if (norm && s != 1) return "forced plan: the fused RMSNorm runs on one split";
        if (s > 1 && nkb / s < kBgWaves) return "forced plan: every wave needs a k-block of every split";
        const int kbs = (nkb + s - 1) / s;
        if (kbs * 32 > kBgMaxStageK) return "forced plan: a split's k-range exceeds the staging registers";
        if (tpw > (1 << 16) || bg_lds_bytes(K, s, tpw) > (size_t)kBgLdsMax) return "forced plan: LDS image too large";
        p = BgPlan{};
        p.ntiles = ntiles;
        p.tpw = tpw;
        p.splits = s;
        p.groups = (ntiles + tpw - 1) / tpw;
        p.lds = bg_lds_bytes(K, s, tpw);
    }
    io->tpw = p.tpw;
    io->splits = p.splits;
    io->groups = p.groups;
    io->step_width = bg_launch_width(norm, p.tpw, p.splits, K);
    io->lds_bytes = (int32_t)p.lds;
    io->counter_off = (int64_t)bg_part_bytes(p);
    return nullptr;
}

// NORM is fixed by the role, as in StepRecorder::prepare: no (Epi, NORM) pair the engine does not name
template <class Epi, class TileEpi, bool NORM, typename WT>
static int bgo_launch(const float* x, const float* norm_w, float eps, const void* w, const uint8_t* wscale, int tiled, int K,
                      int B, const Epi& e, const TileEpi& te, const BgPlan& p, void* workspace, hipStream_t s) {
    SLI_HIP((bg_allow_lds<Epi, NORM, WT>()));
    BgIn in{};
    in.x = x;
    in.norm_w = norm_w;
    in.eps = eps;
    in.K = K;
    in.B = B;
    in.ws = (float*)workspace;
    in.counters = (unsigned*)((char*)workspace + bg_part_bytes(p));
    in.wscale = wscale;  // mxfp4: the block scales (null otherwise)
    const WT* wp = (const WT*)w;
    if (tiled) {  // the engine's bg_build_tiles: the same tile kernel and row map, then the image is streamed
        void* img = (char*)workspace + bgo_image_off(p);
        uint8_t* simg = (uint8_t*)img + bg_tiled_mx_bytes(p.ntiles, K);  // mxfp4 only
        SLI_HIP(launch_bg_tile(wp, K, p.ntiles, te, img, s, wscale, simg));
        wp = (const WT*)img;
        if (is_mx<WT>::value) in.wscale = simg;
        in.tiled = 1;
    }
    SLI_HIP(launch_bgemm(wp, in, e, p, s));
    return SLI_OK;
}

template <typename WT>
static int bgo_role(const float* x, const float* norm_w, float eps, const void* w, const float* rs, const uint8_t* wscale,
                    int tiled, int K, int B, const sli_bgemm_epilogue& e, const BgPlan& p, void* workspace, hipStream_t s) {
    switch (e.role) {
        case SLI_BG_QKV: {
            BgEpiQKV<__half> te{};  // the row map the engine tiles with (it does not depend on the cache type)
            te.hq = e.hq;
            te.hkv = e.hkv;
            te.hd = e.hd;
            auto run = [&](auto* kt) -> int {
                using KT = std::remove_pointer_t<decltype(kt)>;
                BgEpiQKV<KT> q{e.q, (KT*)e.kc, (KT*)e.vc, e.pos, 1, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T};
                q.rscale = rs;
                return bgo_launch<BgEpiQKV<KT>, BgEpiQKV<__half>, true, WT>(x, norm_w, eps, w, wscale, tiled, K, B, q, te, p, workspace, s);
            };
            if (e.kv_dtype == SLI_DT_F16) return run((__half*)nullptr);
            if (e.kv_dtype == SLI_DT_F8E4M3) return run((f8e4m3*)nullptr);
            return run((float*)nullptr);
        }
        case SLI_BG_GATE_UP: {
            const BgEpiSwiGLU g{e.act, e.inter, e.act_mode, rs};
            return bgo_launch<BgEpiSwiGLU, BgEpiSwiGLU, true, WT>(x, norm_w, eps, w, wscale, tiled, K, B, g, g, p, workspace, s);
        }
        case SLI_BG_STORE: {
            const BgEpiStore y{e.y, e.resid, rs, e.scale, e.nrows, e.ld};
            return bgo_launch<BgEpiStore, BgEpiStore, false, WT>(x, norm_w, eps, w, wscale, tiled, K, B, y, y, p, workspace, s);
        }
        default: {
            const BgEpiLogits l{e.logits, (unsigned long long*)e.keys_out, e.nrows, e.ld, e.vocab_off, e.key_ld, rs};
            return bgo_launch<BgEpiLogits, BgEpiLogits, true, WT>(x, norm_w, eps, w, wscale, tiled, K, B, l, l, p, workspace, s);
        }
    }
}

// rows of the weight matrix of an epilogue, or -1 (checked by the caller)
static int64_t bgo_rows(const sli_bgemm_epilogue& e) {
    switch (e.role) {
        case SLI_BG_QKV: return ((int64_t)e.hq + 2 * (int64_t)e.hkv) * e.hd;
        case SLI_BG_GATE_UP: return 2 * (int64_t)e.inter;
        case SLI_BG_STORE:
        case SLI_BG_LOGITS: return e.nrows;
        default: return -1;
    }
}

}  // namespace sli

using namespace sli;

extern "C" {

size_t sli_batch_gemm_workspace_bytes(int32_t rows, int32_t K, int32_t B, int32_t norm, int32_t w_dtype, int32_t tiled,
                                      sli_bgemm_plan* plan) {
    if (!plan || rows < 1 || (w_dtype != SLI_DT_F16 && w_dtype != SLI_DT_I8)) return 0;
    BgPlan p;
    if (const char* why = bgo_plan((rows + 15) / 16, K, B, norm != 0, plan, p)) {
        fail(SLI_ERR_ARG, std::string("sli_batch_gemm_workspace_bytes: ") + why);
        return 0;
    }
    return bgo_ws_bytes(p, K, w_dtype == SLI_DT_I8 ? 1 : 2, tiled);
}

}  // extern "C"

// sli_batch_gemm and sli_batch_gemm_mxfp4 (fn: the entry's name in messages; mx_scales: the block scales of an
// SLI_DT_MXFP4 matrix, null for the other weight types): one contract, one body
static int bgo_entry(const std::string& fn, const float* x, const float* norm_w, float eps, const void* w, int w_dtype,
                     const float* w_row_scale, const void* mx_scales, int32_t tiled, int32_t K, int32_t B,
                     const sli_bgemm_epilogue* epi, sli_bgemm_plan* plan, void* workspace, size_t workspace_bytes,
                     sli_stream_t stream) {
    const bool mx = w_dtype == SLI_DT_MXFP4;
    SLI_CHECK(x && w && epi && plan && workspace && (!mx || mx_scales), SLI_ERR_ARG, fn + ": null pointer");
    SLI_CHECK(bgo_al16(x) && bgo_al16(norm_w) && bgo_al16(w) && bgo_al16(w_row_scale) && bgo_al16(mx_scales) &&
                  bgo_al16(workspace),
              SLI_ERR_ARG, fn + ": 16-byte alignment");
    const sli_bgemm_epilogue& e = *epi;
    const bool norm = norm_w != nullptr;
    switch (e.role) {
        case SLI_BG_QKV:
            SLI_CHECK(norm, SLI_ERR_ARG, fn + ": the q/k/v launch has the fused RMSNorm (norm_w)");
            SLI_CHECK(e.q && e.kc && e.vc && e.pos && e.sin_t && e.cos_t, SLI_ERR_ARG, fn + ": null q/k/v operand");
            SLI_CHECK(e.kv_dtype == SLI_DT_F32 || e.kv_dtype == SLI_DT_F16 || e.kv_dtype == SLI_DT_F8E4M3, SLI_ERR_ARG,
                      fn + ": bad kv dtype");
            SLI_CHECK(e.hd == 64 || e.hd == 128, SLI_ERR_ARG, fn + ": head_dim must be 64 or 128");
            SLI_CHECK(e.hq >= 1 && e.hkv >= 1 && e.hq % e.hkv == 0 && e.hq <= (1 << 16), SLI_ERR_ARG,
                      fn + ": hq must be a multiple of hkv");
            SLI_CHECK(bgo_rows(e) % 16 == 0, SLI_ERR_ARG, fn + ": (hq + 2 hkv) * hd must be a multiple of 16");
            SLI_CHECK(e.T >= 1 && (int64_t)e.T * e.hd * e.hkv * kBgMaxBatch < ((int64_t)1 << 40), SLI_ERR_ARG,
                      fn + ": T must be positive");
            SLI_CHECK(bgo_al16(e.q) && bgo_al16(e.kc) && bgo_al16(e.vc) && bgo_al16(e.pos) && bgo_al16(e.sin_t) &&
                          bgo_al16(e.cos_t),
                      SLI_ERR_ARG, fn + ": 16-byte alignment");
            break;
        case SLI_BG_GATE_UP:
            SLI_CHECK(norm, SLI_ERR_ARG, fn + ": the gate/up launch has the fused RMSNorm (norm_w)");
            SLI_CHECK(e.act, SLI_ERR_ARG, fn + ": null act");
            SLI_CHECK(e.inter >= 8 && e.inter % 8 == 0 && e.inter <= (1 << 28), SLI_ERR_ARG,
                      fn + ": inter must be a positive multiple of 8");
            SLI_CHECK(e.act_mode == 0 || e.act_mode == 1, SLI_ERR_ARG, fn + ": act_mode must be 0 or 1");
            SLI_CHECK(bgo_al16(e.act), SLI_ERR_ARG, fn + ": 16-byte alignment");
            break;
        case SLI_BG_STORE:
            SLI_CHECK(!norm, SLI_ERR_ARG, fn + ": the store launch (wo / down) has no fused RMSNorm");
            SLI_CHECK(e.y, SLI_ERR_ARG, fn + ": null y");
            SLI_CHECK(e.nrows >= 1 && e.ld >= e.nrows, SLI_ERR_ARG, fn + ": ld must be >= nrows >= 1");
            SLI_CHECK(bgo_al16(e.y) && bgo_al16(e.resid), SLI_ERR_ARG, fn + ": 16-byte alignment");
            break;
        case SLI_BG_LOGITS:
            SLI_CHECK(norm, SLI_ERR_ARG, fn + ": the LM head launch has the fused RMSNorm (norm_w)");
            SLI_CHECK(e.logits && e.keys_out, SLI_ERR_ARG, fn + ": null logits operand");
            SLI_CHECK(e.nrows >= 1 && e.ld >= e.nrows, SLI_ERR_ARG, fn + ": ld must be >= nrows >= 1");
            SLI_CHECK(e.vocab_off >= 0 && (int64_t)e.vocab_off + e.nrows <= 0x7FFFFFFF, SLI_ERR_ARG,
                      fn + ": vocab_off must be >= 0");
            SLI_CHECK(bgo_al16(e.logits) && bgo_al16(e.keys_out), SLI_ERR_ARG, fn + ": 16-byte alignment");
            break;
        default: return fail(SLI_ERR_ARG, fn + ": role must be 0 (q/k/v), 1 (gate/up), 2 (store) or 3 (logits)");
    }
    const int64_t rows = bgo_rows(e);
    SLI_CHECK(rows >= 1 && rows <= 0x7FFFFFF0, SLI_ERR_ARG, fn + ": bad row count");
    BgPlan p;
    if (const char* why = bgo_plan((int)((rows + 15) / 16), K, B, norm, plan, p))
        return fail(SLI_ERR_ARG, fn + ": " + why);
    SLI_CHECK(e.role != SLI_BG_LOGITS || e.key_ld >= p.groups, SLI_ERR_ARG,
              fn + ": key_ld must hold one key per workgroup group");
    SLI_CHECK(workspace_bytes >= (mx ? bgo_ws_bytes_mx(p, K, tiled) : bgo_ws_bytes(p, K, w_dtype == SLI_DT_I8 ? 1 : 2, tiled)),
              SLI_ERR_ARG,
              fn + ": workspace too small");
    hipStream_t s = as_stream(stream);
    if (mx)
        return bgo_role<mxfp4>(x, norm_w, eps, w, nullptr, (const uint8_t*)mx_scales, tiled, K, B, e, p, workspace, s);
    if (w_dtype == SLI_DT_I8)
        return bgo_role<int8_t>(x, norm_w, eps, w, w_row_scale, nullptr, tiled, K, B, e, p, workspace, s);
    return bgo_role<__half>(x, norm_w, eps, w, w_row_scale, nullptr, tiled, K, B, e, p, workspace, s);
}

extern "C" {

int sli_batch_gemm(const float* x, const float* norm_w, float eps, const void* w, int w_dtype, const float* w_row_scale,
                   int32_t tiled, int32_t K, int32_t B, const sli_bgemm_epilogue* epi, sli_bgemm_plan* plan,
                   void* workspace, size_t workspace_bytes, sli_stream_t stream) {
    SLI_CHECK(w_dtype == SLI_DT_F16 || w_dtype == SLI_DT_I8, SLI_ERR_ARG, "sli_batch_gemm: fp16 or int8 weights");
    return bgo_entry("sli_batch_gemm", x, norm_w, eps, w, w_dtype, w_row_scale, nullptr, tiled, K, B, epi, plan, workspace,
                     workspace_bytes, stream);
}

size_t sli_batch_gemm_mxfp4_workspace_bytes(int32_t rows, int32_t K, int32_t B, int32_t norm, int32_t tiled,
                                            sli_bgemm_plan* plan) {
    if (!plan || rows < 1) return 0;
    BgPlan p;
    if (const char* why = bgo_plan((rows + 15) / 16, K, B, norm != 0, plan, p)) {
        fail(SLI_ERR_ARG, std::string("sli_batch_gemm_mxfp4_workspace_bytes: ") + why);
        return 0;
    }
    return bgo_ws_bytes_mx(p, K, tiled);
}

int sli_batch_gemm_mxfp4(const float* x, const float* norm_w, float eps, const void* data, const void* scales,
                         int32_t tiled, int32_t K, int32_t B, const sli_bgemm_epilogue* epi, sli_bgemm_plan* plan,
                         void* workspace, size_t workspace_bytes, sli_stream_t stream) {
    return bgo_entry("sli_batch_gemm_mxfp4", x, norm_w, eps, data, SLI_DT_MXFP4, nullptr, scales, tiled, K, B, epi, plan,
                     workspace, workspace_bytes, stream);
}

// The plain-rows projection: the store role with no residual and scale 1, the planner's plan, counters zeroed here
size_t sli_matmul_batch_mxfp4_workspace_bytes(int32_t rows, int32_t cols, int32_t batch, int32_t tiled) {
    if (rows <= 0 || cols <= 0 || batch <= 0 || batch > kBgMaxBatch || cols % 32 != 0) return 0;
    const BgPlan p = bg_plan((rows + 15) / 16, cols, batch, false, device_cus());
    if (p.groups <= 0) return 0;
    return bgo_ws_bytes_mx(p, cols, tiled);
}

int sli_matmul_batch_mxfp4(const float* x, const void* data, const void* scales, float* y, int32_t rows, int32_t cols,
                           int32_t batch, int32_t tiled, void* workspace, size_t workspace_bytes, sli_stream_t stream) {
    SLI_CHECK(x && data && scales && y && workspace, SLI_ERR_ARG, "sli_matmul_batch_mxfp4: null pointer");
    SLI_CHECK(rows > 0 && cols > 0 && cols % 32 == 0, SLI_ERR_SHAPE, "sli_matmul_batch_mxfp4: cols must be a multiple of 32");
    SLI_CHECK(batch >= 1 && batch <= kBgMaxBatch, SLI_ERR_SHAPE, "sli_matmul_batch_mxfp4: batch must be in [1, 8]");
    SLI_CHECK(bgo_al16(x) && bgo_al16(data) && bgo_al16(scales) && bgo_al16(y) && bgo_al16(workspace), SLI_ERR_ARG,
              "sli_matmul_batch_mxfp4: 16-byte alignment");
    const BgPlan p = bg_plan((rows + 15) / 16, cols, batch, false, device_cus());
    SLI_CHECK(p.groups > 0, SLI_ERR_SHAPE, "sli_matmul_batch_mxfp4: no tiling fits");
    SLI_CHECK(workspace_bytes >= bgo_ws_bytes_mx(p, cols, tiled), SLI_ERR_ARG, "sli_matmul_batch_mxfp4: workspace too small");
    hipStream_t s = as_stream(stream);
    SLI_HIP(hipMemsetAsync((char*)workspace + bg_part_bytes(p), 0, sizeof(unsigned) * p.groups, s));
    const BgEpiStore e{y, nullptr, nullptr, 1.0f, rows, rows};
    return bgo_launch<BgEpiStore, BgEpiStore, false, mxfp4>(x, nullptr, 0.0f, data, (const uint8_t*)scales, tiled, cols, batch,
                                                            e, e, p, workspace, s);
}

}  // extern "C"
