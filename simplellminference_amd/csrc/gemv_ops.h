// gemv_ops.h — one batch-1 decode GEMV launch as a kernel-level entry point (include/sli.h "decode stages, for tests
// and labs"): one gemv_kernel / gemv_merge_kernel / gemv_sum_kernel launch (gemv.h) on caller-provided device buffers,
// with the input staging, epilogue, weight type, cache type and schedule of any launch StepRecorder<WT, KT> records
// for batch 1. Included once, at the end of engine.hip, and written over the engine's own template arguments (the
// launch_gemv* calls below are StepRecorder's, argument for argument), so the library holds ONE compiled copy of every
// GEMV kernel and the entry launches the very code objects a model step launches; role, staging and norm are paired as
// the engine pairs them, which keeps that set closed. The GEMVs keep no counters: no model, no workspace.
//
// The plan (sli_gemv_plan) is made by the engine's own planners (gemv_split, gemv_blocks, gemv_balanced_blocks,
// gemv_wave_count, gemv_ksplit_grid) as if the chip had `cus` compute units: their workgroup cap is a host argument,
// so a matrix of a few hundred rows runs the schedule an 11008-row one runs on 256 CUs (several units per wave,
// unequal waves, the balanced grid). Whatever the kernels would read or write out of bounds for is refused here,
// before anything touches the device.
//
// Not covered: EpiPush (the residual exchange inside wo / down needs peers), the shared q/k/v + attention launch
// (qkv_attn.h; tests/test_gpu_qkv_attn.py holds it bit for bit to the two-launch step) and tp_layers.h.
#pragma once
#include "common.h"
#include "gemv.h"

namespace sli {

static bool gvo_al16(const void* p) { return (uintptr_t)p % 16 == 0; }

struct GvoArgs {
    const float* x;
    const float* norm_w;
    float eps;
    const void* w;
    const float* rs;         // row scales (f32 / f16 / int8 weights; nullable)
    const uint8_t* wscale;   // mxfp4 block scales
    int cols;
    const sli_gemv_epilogue* e;
    int maxb;
    GemvRan* ran;
    hipStream_t s;
};

template <typename WT>
static GemvIn gvo_in(const GvoArgs& a, const float* x, const float* norm_w, int cols) {
    GemvIn in{x, norm_w, norm_w ? a.eps : 0.0f, cols};
    if (is_mx<WT>::value) in.wscale = a.wscale;
    return in;
}

// StepRecorder<WT, KT>::gemv_qkv
template <typename WT, typename KT>
static hipError_t gvo_qkv(const GvoArgs& a) {
    const sli_gemv_epilogue& e = *a.e;
    const GemvIn in = gvo_in<WT>(a, a.x, a.norm_w, a.cols);
    EpiQKV<KT> q{e.q, (KT*)e.kc, (KT*)e.vc, a.rs, e.pos, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T};
    return launch_gemv_u<WT, 2, 4, true>((const WT*)a.w, in, q, (e.hq + 2 * e.hkv) * (e.hd / 2), a.s, a.maxb, a.ran);
}

// StepRecorder::gemv_gu
template <typename WT>
static hipError_t gvo_gate_up(const GvoArgs& a) {
    const sli_gemv_epilogue& e = *a.e;
    const GemvIn in = gvo_in<WT>(a, a.x, a.norm_w, a.cols);
    const EpiSwiGLU g{e.act, a.rs, e.inter, e.act_mode};
    constexpr int UG = gemv_uw<WT, 4>();
    if (e.np == 2)
        return launch_gemv_sum<WT, 2, UG, true, EpiSwiGLU, 2>((const WT*)a.w, in, g, e.parts, e.inter, a.s, a.maxb, a.ran);
    if (e.np == 4)
        return launch_gemv_sum<WT, 2, UG, true, EpiSwiGLU, 4>((const WT*)a.w, in, g, e.parts, e.inter, a.s, a.maxb, a.ran);
    return launch_gemv_u<WT, 2, 4, true>((const WT*)a.w, in, g, e.inter, a.s, a.maxb, a.ran);
}

// StepRecorder::gemv_wo / gemv_wo_ks
template <typename WT>
static hipError_t gvo_wo(const GvoArgs& a) {
    constexpr bool MX = is_mx<WT>::value, I8 = std::is_same<WT, int8_t>::value;
    const sli_gemv_epilogue& e = *a.e;
    const WT* w = (const WT*)a.w;
    if (!e.part) {  // the attention merged its splits: a plain input
        const GemvIn in = gvo_in<WT>(a, a.x, nullptr, a.cols);
        const EpiStore<1> y{e.y, e.resid, a.rs, 1.0f, e.nrows};
        return launch_gemv_u<WT, 1, 2, true>(w, in, y, e.nrows, a.s, a.maxb, a.ran);
    }
    AttnMergeIn am{e.part, e.pos, e.max_splits, e.ppwg, e.hd};
    if (e.ks > 1) {
        const GemvIn in = gvo_in<WT>(a, nullptr, nullptr, a.cols / e.ks);
        const EpiKPart k{e.kpart, a.rs, e.nrows, e.ks};
        am.ksplit = e.ks;
        am.kunits = e.nrows;
        const int grid = gemv_ksplit_grid(e.nrows, e.ks, a.maxb);
        constexpr int UK = MX ? kMxWoU : I8 ? 1 : 2, NBK = MX ? kMxWoNB : I8 ? 2 : 4;
        if (am.max_splits > 8) return launch_gemv_merge_ks<WT, 1, UK, true, EpiKPart, 16, NBK>(w, in, k, am, grid, a.s, a.ran);
        return launch_gemv_merge_ks<WT, 1, UK, true, EpiKPart, 8, NBK>(w, in, k, am, grid, a.s, a.ran);
    }
    const GemvIn in = gvo_in<WT>(a, nullptr, nullptr, a.cols);
    const EpiStore<1> y{e.y, e.resid, a.rs, 1.0f, e.nrows};
    constexpr int UW = MX ? kMxWoU : 2;
    if (am.max_splits > 8)
        return launch_gemv_merge<WT, 1, UW, true, EpiStore<1>, 16>(w, in, y, am, e.nrows, a.s, a.maxb, a.ran);
    return launch_gemv_merge<WT, 1, UW, true>(w, in, y, am, e.nrows, a.s, a.maxb, a.ran);
}

// StepRecorder::gemv_down / gemv_down_sum
template <typename WT, class Epi>
static hipError_t gvo_down_epi(const GvoArgs& a, const Epi& y) {
    const GemvIn in = gvo_in<WT>(a, a.x, nullptr, a.cols);
    if constexpr (std::is_same<WT, int8_t>::value)
        return launch_gemv<WT, 1, 4, true>((const WT*)a.w, in, y, a.e->nrows, a.s, a.maxb, a.ran);
    else
        return launch_gemv_u<WT, 1, 6, true>((const WT*)a.w, in, y, a.e->nrows, a.s, a.maxb, a.ran);
}
template <typename WT>
static hipError_t gvo_down(const GvoArgs& a) {
    const sli_gemv_epilogue& e = *a.e;
    if (e.np == 2) return gvo_down_epi<WT>(a, EpiStoreSum<1, 2>{e.y, e.resid, e.parts, a.rs, e.nrows});
    if (e.np == 4) return gvo_down_epi<WT>(a, EpiStoreSum<1, 4>{e.y, e.resid, e.parts, a.rs, e.nrows});
    return gvo_down_epi<WT>(a, EpiStore<1>{e.y, e.resid, a.rs, 1.0f, e.nrows});
}

// StepRecorder::gemv_lm
template <typename WT>
static hipError_t gvo_logits(const GvoArgs& a) {
    const sli_gemv_epilogue& e = *a.e;
    const GemvIn in = gvo_in<WT>(a, a.x, a.norm_w, a.cols);
    const EpiLogits<2> l{e.logits, (unsigned long long*)e.keys, a.rs, e.nrows, e.vocab_off, 0ull};
    return launch_gemv_u<WT, 2, 4, true>((const WT*)a.w, in, l, (e.nrows + 1) / 2, a.s, a.maxb, a.ran);
}

// the (WT, KT) pairs of engine.hip's dispatch table (SLI_DISPATCH): every pair but fp32 weights with an FP8 cache
template <typename WT>
static hipError_t gvo_role(const GvoArgs& a) {
    switch (a.e->role) {
        case SLI_GV_QKV:
            if (a.e->kv_dtype == SLI_DT_F16) return gvo_qkv<WT, __half>(a);
            if constexpr (!std::is_same<WT, float>::value) {
                if (a.e->kv_dtype == SLI_DT_F8E4M3) return gvo_qkv<WT, f8e4m3>(a);
            }
            return gvo_qkv<WT, float>(a);
        case SLI_GV_GATE_UP: return gvo_gate_up<WT>(a);
        case SLI_GV_WO: return gvo_wo<WT>(a);
        case SLI_GV_DOWN: return gvo_down<WT>(a);
        default: return gvo_logits<WT>(a);
    }
}

static hipError_t gvo_dispatch(int w_dtype, const GvoArgs& a) {
    if (w_dtype == SLI_DT_MXFP4) return gvo_role<mxfp4>(a);
    if (w_dtype == SLI_DT_I8) return gvo_role<int8_t>(a);
    if (w_dtype == SLI_DT_F16) return gvo_role<__half>(a);
    return gvo_role<float>(a);
}

static int gvo_epv(int w_dtype) { return w_dtype == SLI_DT_MXFP4 ? 32 : w_dtype == SLI_DT_I8 ? 16 : w_dtype == SLI_DT_F16 ? 8 : 4; }

// rows of the weight matrix of an epilogue
static int64_t gvo_rows(const sli_gemv_epilogue& e) {
    switch (e.role) {
        case SLI_GV_QKV: return ((int64_t)e.hq + 2 * (int64_t)e.hkv) * e.hd;
        case SLI_GV_GATE_UP: return 2 * (int64_t)e.inter;
        default: return e.nrows;
    }
}

// Everything that needs no pointer: the shape, the role's pairing and the plan. nullptr and *ran resolved (dry), or
// the refusal. with_device: cus is also held to the device's CU count.
static const char* gvo_resolve(int w_dtype, int cols, bool norm, const sli_gemv_epilogue& e, sli_gemv_plan* io,
                               bool with_device, GemvRan& ran) {
    if (w_dtype != SLI_DT_F32 && w_dtype != SLI_DT_F16 && w_dtype != SLI_DT_I8 && w_dtype != SLI_DT_MXFP4)
        return "bad weight dtype";
    const int epv = gvo_epv(w_dtype);
    if (cols < epv || cols % epv != 0)
        return "cols must be a positive multiple of the weight type's vector width (f32 4, f16 8, int8 16, mxfp4 32)";
    if (cols > kGemvMaxCols) return "cols exceeds the staged input (16320)";
    if (io->cus < 0) return "cus must be >= 0";
    if (io->cus > 0 && with_device && io->cus > device_cus()) return "cus exceeds the device's compute units";
    if (io->cus > 4096) return "cus exceeds 4096";
    switch (e.role) {
        case SLI_GV_QKV:
            if (!norm) return "the q/k/v launch has the fused RMSNorm (norm_w)";
            if (e.np != 0 || e.part) return "the q/k/v launch stages a plain input";
            if (e.kv_dtype != SLI_DT_F32 && e.kv_dtype != SLI_DT_F16 && e.kv_dtype != SLI_DT_F8E4M3) return "bad kv dtype";
            if (w_dtype == SLI_DT_F32 && e.kv_dtype == SLI_DT_F8E4M3) return "the engine pairs no fp32 weights with an FP8 cache";
            if (e.hd != 64 && e.hd != 128) return "head_dim must be 64 or 128";
            if (e.hq < 1 || e.hkv < 1 || e.hq % e.hkv != 0 || e.hq > (1 << 12)) return "hq must be a multiple of hkv";
            if (e.T < 1 || (int64_t)e.T * e.hd * e.hkv >= ((int64_t)1 << 31)) return "T must be positive (and one layer's cache below 2^31 elements)";
            break;
        case SLI_GV_GATE_UP:
            if (!norm) return "the gate/up launch has the fused RMSNorm (norm_w)";
            if (e.part) return "the gate/up launch stages x, or x plus the K-split partials";
            if (e.np != 0 && e.np != 2 && e.np != 4) return "np must be 0, 2 or 4";
            if (e.np != 0 && cols > 4 * kGemvThreads) return "x plus partials is staged in one round: cols <= 4096";
            if (e.inter < 1) return "inter must be positive";
            if (e.act_mode != 0 && e.act_mode != 1) return "act_mode must be 0 or 1";
            break;
        case SLI_GV_WO:
            if (norm) return "the wo launch has no fused RMSNorm";
            if (e.np != 0) return "the wo launch takes no partials to add (np)";
            if (e.nrows < 1) return "nrows must be positive";
            if (!e.part) {
                if (e.ks > 1) return "the K-split wo merges its input from the attention's partials (part)";
                break;
            }
            if (e.hd != 64 && e.hd != 128) return "head_dim must be 64 or 128";
            if (e.hq < 1 || (int64_t)e.hq * e.hd != cols) return "merged input: cols must be hq * hd";
            if (e.max_splits < 1 || e.max_splits > (1 << 16) || e.ppwg < 1) return "max_splits and ppwg must be positive";
            if (e.ks > 1) {
                if (e.ks != 2 && e.ks != 4) return "ks must be 1, 2 or 4";
                if (e.hq % e.ks != 0) return "K-split: hq must be a multiple of ks";
                if ((cols / e.ks) % epv != 0) return "K-split: cols / ks must be a multiple of the weight type's vector width";
                if (gemv_ksplit_grid(e.nrows, e.ks, io->cus ? io->cus : gemv_max_blocks()) == 0)
                    return "K-split: no grid keeps every workgroup inside one column block";
            }
            break;
        case SLI_GV_DOWN:
            if (norm) return "the down launch has no fused RMSNorm";
            if (e.part) return "the down launch stages a plain input";
            if (e.np != 0 && e.np != 2 && e.np != 4) return "np must be 0, 2 or 4";
            if (e.nrows < 1) return "nrows must be positive";
            break;
        case SLI_GV_LOGITS:
            if (!norm) return "the LM head launch has the fused RMSNorm (norm_w)";
            if (e.np != 0 || e.part) return "the LM head launch stages a plain input";
            if (e.nrows < 1) return "nrows must be positive";
            if (e.vocab_off < 0 || (int64_t)e.vocab_off + e.nrows > 0x7FFFFFFF) return "vocab_off must be >= 0";
            break;
        default: return "role must be 0 (q/k/v), 1 (gate/up), 2 (wo), 3 (down) or 4 (logits)";
    }
    const int64_t rows = gvo_rows(e);
    // (gemv_block's unit partition is 32-bit: grid waves x units stays below 2^32)
    if (rows < 1 || rows * (e.role == SLI_GV_WO && e.ks > 1 ? e.ks : 1) >= (1 << 20)) return "bad row count (at most 2^20 - 1 units)";
    ran = GemvRan{};
    ran.dry = true;
    GvoArgs a{};
    a.cols = cols;
    a.e = &e;
    a.maxb = io->cus ? io->cus : gemv_max_blocks();
    a.ran = &ran;
    static const float one = 1.0f;
    a.norm_w = norm ? &one : nullptr;  // (dry: only its presence matters)
    if (gvo_dispatch(w_dtype, a) != hipSuccess || ran.grid < 1) return "no launch for this shape";
    if (ran.lds > 64 * 1024) return "the staged input and the workgroup's row sums exceed 64 KiB of LDS";
    if (e.role == SLI_GV_LOGITS && e.key_ld < ran.grid && with_device) return "key_ld must hold one key per workgroup";
    io->grid = ran.grid;
    io->units = ran.units;
    io->csplit = ran.csplit;
    io->u = ran.u;
    io->chunks_per_row = ran.cpr;
    io->chunks_per_part = ran.cpp;
    io->cw = ran.cw;
    io->nb = ran.nb;
    io->ns = ran.ns;
    io->masked_tail = ran.masked;
    io->lds_bytes = (int32_t)ran.lds;
    return nullptr;
}

static int gvo_entry(const std::string& fn, const float* x, const float* norm_w, float eps, const void* w, int w_dtype,
                     const float* rs, const void* mx_scales, int32_t cols, const sli_gemv_epilogue* epi,
                     sli_gemv_plan* plan, sli_stream_t stream) {
    const bool mx = w_dtype == SLI_DT_MXFP4;
    SLI_CHECK(w && epi && plan && (!mx || mx_scales), SLI_ERR_ARG, fn + ": null pointer");
    const sli_gemv_epilogue& e = *epi;
    SLI_CHECK(gvo_al16(x) && gvo_al16(norm_w) && gvo_al16(w) && gvo_al16(rs) && gvo_al16(mx_scales) && gvo_al16(e.parts) &&
                  gvo_al16(e.part) && gvo_al16(e.pos) && gvo_al16(e.q) && gvo_al16(e.kc) && gvo_al16(e.vc) &&
                  gvo_al16(e.sin_t) && gvo_al16(e.cos_t) && gvo_al16(e.act) && gvo_al16(e.y) && gvo_al16(e.resid) &&
                  gvo_al16(e.kpart) && gvo_al16(e.logits) && gvo_al16(e.keys),
              SLI_ERR_ARG, fn + ": 16-byte alignment");
    GemvRan ran;
    if (const char* why = gvo_resolve(w_dtype, cols, norm_w != nullptr, e, plan, true, ran))
        return fail(SLI_ERR_ARG, fn + ": " + why);
    const bool merged = e.role == SLI_GV_WO && e.part;
    SLI_CHECK(merged ? e.pos != nullptr : x != nullptr, SLI_ERR_ARG, fn + ": null input");
    SLI_CHECK(e.np == 0 || e.parts, SLI_ERR_ARG, fn + ": null partials");
    switch (e.role) {
        case SLI_GV_QKV:
            SLI_CHECK(e.q && e.kc && e.vc && e.pos && e.sin_t && e.cos_t, SLI_ERR_ARG, fn + ": null q/k/v operand");
            break;
        case SLI_GV_GATE_UP: SLI_CHECK(e.act, SLI_ERR_ARG, fn + ": null act"); break;
        case SLI_GV_WO:
            SLI_CHECK(e.ks > 1 ? e.kpart != nullptr : e.y != nullptr, SLI_ERR_ARG, fn + ": null output");
            break;
        case SLI_GV_DOWN:
            SLI_CHECK(e.y, SLI_ERR_ARG, fn + ": null output");
            SLI_CHECK(e.np == 0 || e.resid, SLI_ERR_ARG, fn + ": the summed residual needs x (resid)");
            break;
        default: SLI_CHECK(e.logits && e.keys, SLI_ERR_ARG, fn + ": null logits operand"); break;
    }
    GvoArgs a{x, norm_w, eps, w, mx ? nullptr : rs, (const uint8_t*)mx_scales, cols, &e, plan->cus ? plan->cus : gemv_max_blocks(),
              nullptr, as_stream(stream)};
    SLI_HIP(gvo_dispatch(w_dtype, a));
    return SLI_OK;
}

}  // namespace sli

using namespace sli;

extern "C" {

int sli_decode_gemv_plan(int w_dtype, int32_t cols, int32_t norm, const sli_gemv_epilogue* epi, sli_gemv_plan* plan) {
    SLI_CHECK(epi && plan, SLI_ERR_ARG, "sli_decode_gemv_plan: null pointer");
    GemvRan ran;
    if (const char* why = gvo_resolve(w_dtype, cols, norm != 0, *epi, plan, false, ran))
        return fail(SLI_ERR_ARG, std::string("sli_decode_gemv_plan: ") + why);
    return SLI_OK;
}

int sli_decode_gemv(const float* x, const float* norm_w, float eps, const void* w, int w_dtype, const float* w_row_scale,
                    int32_t cols, const sli_gemv_epilogue* epi, sli_gemv_plan* plan, sli_stream_t stream) {
    SLI_CHECK(w_dtype == SLI_DT_F32 || w_dtype == SLI_DT_F16 || w_dtype == SLI_DT_I8, SLI_ERR_ARG,
              "sli_decode_gemv: fp32, fp16 or int8 weights");
    return gvo_entry("sli_decode_gemv", x, norm_w, eps, w, w_dtype, w_row_scale, nullptr, cols, epi, plan, stream);
}

int sli_decode_gemv_mxfp4(const float* x, const float* norm_w, float eps, const void* data, const void* scales,
                          int32_t cols, const sli_gemv_epilogue* epi, sli_gemv_plan* plan, sli_stream_t stream) {
    return gvo_entry("sli_decode_gemv_mxfp4", x, norm_w, eps, data, SLI_DT_MXFP4, nullptr, scales, cols, epi, plan, stream);
}

}  // extern "C"
