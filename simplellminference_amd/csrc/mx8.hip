// mx8.hip — the MXFP8 activation format and the block-scaled MFMA kernels (the prefill GEMM of pgemm_mx8.h, the batched
// decode projection of bgemm_mx8.h) as entry points of the C ABI (include/sli.h): the format's quantise / dequantise
// ops, the two quantising producers, one GEMM launch and one batched projection launch. A translation unit of its own:
// it holds the one compiled copy of every pgemm_mx8 and bgemm_mx8 kernel.
#include "mx8_api.h"
#include "bgemm_mx8.h"
#include "pgemm_mx8.h"

namespace sli {

static bool mx8_al(const void* p, uintptr_t a) { return (uintptr_t)p % a == 0; }

template <class Src, bool NORM>
static int mx8_quant_launch(const Src& src, const float* w, void* codes, void* scales, int rows, int D, float eps,
                            hipStream_t s) {
    hipLaunchKernelGGL((pf_quant_mx8_kernel<Src, NORM>), dim3(rows), dim3(256), 0, s, src, w, (uint8_t*)codes,
                       (uint8_t*)scales, D, eps);
    SLI_HIP(hipGetLastError());
    return SLI_OK;
}

template <class Epi>
static int mx8_gemm_launch(const Pg8In& in, int role, const Epi& e, sli_pgemm_tiling* tiling, hipStream_t s) {
    return pg8_pick(in.M, role, [&](auto cfg) -> int {
        using Cfg = decltype(cfg);
        if (tiling) *tiling = sli_pgemm_tiling{Cfg::BM, Cfg::WR, Cfg::S, Cfg::AT, 1, 0, Pg8Geo<Cfg>::KS};
        SLI_HIP((launch_pgemm_mx8<Epi, Cfg>(in, e, s)));
        return SLI_OK;
    });
}

static int mx8_gemm_role(const Pg8In& in, const sli_pgemm_epilogue& e, const PfSegs* segs, sli_pgemm_tiling* tiling,
                         hipStream_t s) {
    if (e.role == 0) {
        if (e.kv_dtype == SLI_DT_F8E4M3) {
            const PgEpiQKV<f8e4m3> q{e.q, (f8e4m3*)e.kc, (f8e4m3*)e.vc, nullptr, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T, segs};
            return mx8_gemm_launch(in, 0, q, tiling, s);
        }
        if (e.kv_dtype == SLI_DT_F16) {
            const PgEpiQKV<__half> q{e.q, (__half*)e.kc, (__half*)e.vc, nullptr, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T, segs};
            return mx8_gemm_launch(in, 0, q, tiling, s);
        }
        const PgEpiQKV<float> q{e.q, (float*)e.kc, (float*)e.vc, nullptr, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T, segs};
        return mx8_gemm_launch(in, 0, q, tiling, s);
    }
    if (e.role == 1) {
        const PgEpiSwiGLU g{(__half*)e.ahi, (__half*)e.alo, nullptr, e.inter, e.act_mode};
        return mx8_gemm_launch(in, 1, g, tiling, s);
    }
    if (e.role == 3) {  // any N >= 16: the launch covers whole 16-row tiles, the epilogue masks at N
        const PgEpiLogits g{e.y, nullptr, in.N, e.ld};
        Pg8In up = in;
        up.N = pg_logits_n(in.N);
        return mx8_gemm_launch(up, 3, g, tiling, s);
    }
    const PgEpiResid r{e.y, e.resid, nullptr, in.N, e.ld};
    return mx8_gemm_launch(in, 2, r, tiling, s);
}

int mx8_prepare() {
    static const hipError_t err = [] {
        hipError_t e = pg8_allow_lds_all<PgEpiQKV<f8e4m3>>();
        if (e == hipSuccess) e = pg8_allow_lds_all<PgEpiQKV<__half>>();
        if (e == hipSuccess) e = pg8_allow_lds_all<PgEpiQKV<float>>();
        if (e == hipSuccess) e = pg8_allow_lds_all<PgEpiSwiGLU>();
        if (e == hipSuccess) e = pg8_allow_lds_all<PgEpiResid>();
        if (e == hipSuccess) e = pg8_allow_lds_all<PgEpiLogits>();
        return e;
    }();
    SLI_HIP(err);
    return SLI_OK;
}
int mx8_norm_quant(const float* x, const float* w, void* codes, void* scales, int M, int D, float eps, hipStream_t s) {
    const Mx8SrcF32 src{x};
    if (w) return mx8_quant_launch<Mx8SrcF32, true>(src, w, codes, scales, M, D, eps, s);
    return mx8_quant_launch<Mx8SrcF32, false>(src, nullptr, codes, scales, M, D, eps, s);
}
int mx8_pair_quant(const void* hi, const void* lo, void* codes, void* scales, int M, int D, hipStream_t s) {
    const Mx8SrcPair src{(const __half*)hi, (const __half*)lo};
    return mx8_quant_launch<Mx8SrcPair, false>(src, nullptr, codes, scales, M, D, 0.0f, s);
}
int mx8_gemm(const void* data, const void* scales, const void* acodes, const void* ascales, int N, int K, int M,
             const sli_pgemm_epilogue& e, const void* segs, sli_pgemm_tiling* tiling, hipStream_t s) {
    const Pg8In in{(const uint8_t*)data, (const uint8_t*)scales, (const uint8_t*)acodes, (const uint8_t*)ascales, N, K, M};
    return mx8_gemm_role(in, e, (const PfSegs*)segs, tiling, s);
}

// ---------------------------------------------------------------- the batched decode projection (bgemm_mx8.h)
int mx8_bgemm_prepare() {
    static const hipError_t err = [] {
        hipError_t e = bg8_allow_lds<BgEpiQKV<float>, true>();
        if (e == hipSuccess) e = bg8_allow_lds<BgEpiQKV<__half>, true>();
        if (e == hipSuccess) e = bg8_allow_lds<BgEpiQKV<f8e4m3>, true>();
        if (e == hipSuccess) e = bg8_allow_lds<BgEpiSwiGLU, true>();
        if (e == hipSuccess) e = bg8_allow_lds<BgEpiLogits, true>();
        if (e == hipSuccess) e = bg8_allow_lds<BgEpiStore, false>();
        return e;
    }();
    SLI_HIP(err);
    return SLI_OK;
}
template <class Epi>
static int mx8_bgemm_launch(const Bg8In& in, const Epi& e, const Bg8Plan& p, hipStream_t s) {
    SLI_HIP(launch_bgemm_mx8(in, e, p, s));
    return SLI_OK;
}
int mx8_bgemm(const Bg8In& in, const BgEpiQKV<float>& e, const Bg8Plan& p, hipStream_t s) { return mx8_bgemm_launch(in, e, p, s); }
int mx8_bgemm(const Bg8In& in, const BgEpiQKV<__half>& e, const Bg8Plan& p, hipStream_t s) { return mx8_bgemm_launch(in, e, p, s); }
int mx8_bgemm(const Bg8In& in, const BgEpiQKV<f8e4m3>& e, const Bg8Plan& p, hipStream_t s) { return mx8_bgemm_launch(in, e, p, s); }
int mx8_bgemm(const Bg8In& in, const BgEpiStore& e, const Bg8Plan& p, hipStream_t s) { return mx8_bgemm_launch(in, e, p, s); }
int mx8_bgemm(const Bg8In& in, const BgEpiSwiGLU& e, const Bg8Plan& p, hipStream_t s) { return mx8_bgemm_launch(in, e, p, s); }
int mx8_bgemm(const Bg8In& in, const BgEpiLogits& e, const Bg8Plan& p, hipStream_t s) { return mx8_bgemm_launch(in, e, p, s); }
template <class Epi>
static int mx8_tile_launch(const void* data, const void* scales, int K, int ntiles, const Epi& e, void* out, void* sout,
                           hipStream_t s) {
    SLI_HIP(launch_bg8_tile(data, scales, K, ntiles, e, out, sout, s));
    return SLI_OK;
}
int mx8_bg_tile(const void* data, const void* scales, int K, int ntiles, const BgEpiQKV<__half>& e, void* out, void* sout, hipStream_t s) { return mx8_tile_launch(data, scales, K, ntiles, e, out, sout, s); }
int mx8_bg_tile(const void* data, const void* scales, int K, int ntiles, const BgEpiStore& e, void* out, void* sout, hipStream_t s) { return mx8_tile_launch(data, scales, K, ntiles, e, out, sout, s); }
int mx8_bg_tile(const void* data, const void* scales, int K, int ntiles, const BgEpiSwiGLU& e, void* out, void* sout, hipStream_t s) { return mx8_tile_launch(data, scales, K, ntiles, e, out, sout, s); }
int mx8_bg_tile(const void* data, const void* scales, int K, int ntiles, const BgEpiLogits& e, void* out, void* sout, hipStream_t s) { return mx8_tile_launch(data, scales, K, ntiles, e, out, sout, s); }

// Workspace of an op-level call: split partials and arrival counters (bg8_ws_bytes), then for tiled = 1 the data image
// at the next 256-byte boundary and the scale image right behind it
static size_t bg8o_image_off(const Bg8Plan& p) { return (bg8_ws_bytes(p) + 255) & ~(size_t)255; }
static size_t bg8o_ws_bytes(const Bg8Plan& p, int K, int tiled) {
    return tiled ? bg8o_image_off(p) + bg_tiled_mx_bytes(p.ntiles, K) + bg_tiled_mx_scale_bytes(p.ntiles, K) : bg8_ws_bytes(p);
}
// The plan of a launch: io->tpw == 0 asks bg_mx8_plan; otherwise (tpw, splits, wt, wk) is forced after
// bg8_plan_refusal. Returns nullptr and fills p / io, or the refusal (shape: whether it is a shape refusal).
static const char* bg8o_plan(int64_t rows, int K, int B, bool norm, sli_bgemm_mx8_plan* io, Bg8Plan& p) {
    if (rows < 1 || rows > 0x7FFFFFF0) return "bad row count";
    if (K < kBg8Stage || K % kBg8Stage != 0 || K > (1 << 20)) return "K must be a positive multiple of 128 (one MFMA issue)";
    if (B < 1 || B > kBgMaxBatch) return "batch must be in [1, 8]";
    const int ntiles = (int)((rows + 15) / 16);
    if ((int64_t)ntiles * K >= ((int64_t)1 << 36)) return "shape too large";
    if (io->tpw == 0) {
        p = bg_mx8_plan(ntiles, K, B, norm, device_cus());
        if (p.groups <= 0) return "no plan fits";
    } else {
        if (const char* why = bg8_plan_refusal(ntiles, K, norm, io->tpw, io->splits, io->wt, io->wk)) return why;
        p = Bg8Plan{};
        p.ntiles = ntiles;
        p.tpw = io->tpw;
        p.splits = io->splits;
        p.wt = io->wt;
        p.wk = io->wk;
        p.groups = (ntiles + p.tpw - 1) / p.tpw;
        p.lds = bg8_lds_bytes(K, p.splits, p.tpw, p.wk);
    }
    io->tpw = p.tpw;
    io->splits = p.splits;
    io->wt = p.wt;
    io->wk = p.wk;
    io->groups = p.groups;
    io->lds_bytes = (int32_t)p.lds;
    io->counter_off = (int64_t)bg8_part_bytes(p);
    return nullptr;
}

template <class Epi, class TileEpi>
static int bg8o_launch(const float* x, const float* norm_w, float eps, const void* data, const void* scales, int tiled, int K,
                       int B, const Epi& e, const TileEpi& te, const Bg8Plan& p, void* workspace, hipStream_t s) {
    if (int rc = mx8_bgemm_prepare()) return rc;
    Bg8In in{};
    in.x = x;
    in.norm_w = norm_w;
    in.eps = eps;
    in.K = K;
    in.B = B;
    in.ws = (float*)workspace;
    in.counters = (unsigned*)((char*)workspace + bg8_part_bytes(p));
    in.w = (const uint8_t*)data;
    in.wscale = (const uint8_t*)scales;
    if (tiled) {  // the model's re-lay: the same tile kernel and row map, then the images are streamed
        uint8_t* img = (uint8_t*)workspace + bg8o_image_off(p);
        uint8_t* simg = img + bg_tiled_mx_bytes(p.ntiles, K);
        SLI_HIP(launch_bg8_tile(data, scales, K, p.ntiles, te, img, simg, s));
        in.w = img;
        in.wscale = simg;
        in.tiled = 1;
    }
    SLI_HIP(launch_bgemm_mx8(in, e, p, s));
    return SLI_OK;
}

static int bg8o_role(const float* x, const float* norm_w, float eps, const void* data, const void* scales, int tiled, int K,
                     int B, const sli_bgemm_epilogue& e, const Bg8Plan& p, void* workspace, hipStream_t s) {
    switch (e.role) {
        case SLI_BG_QKV: {
            BgEpiQKV<__half> te{};  // the row map the model tiles with (it does not depend on the cache type)
            te.hq = e.hq;
            te.hkv = e.hkv;
            te.hd = e.hd;
            auto run = [&](auto* kt) -> int {
                using KT = std::remove_pointer_t<decltype(kt)>;
                const BgEpiQKV<KT> q{e.q, (KT*)e.kc, (KT*)e.vc, e.pos, 1, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T};
                return bg8o_launch(x, norm_w, eps, data, scales, tiled, K, B, q, te, p, workspace, s);
            };
            if (e.kv_dtype == SLI_DT_F16) return run((__half*)nullptr);
            if (e.kv_dtype == SLI_DT_F8E4M3) return run((f8e4m3*)nullptr);
            return run((float*)nullptr);
        }
        case SLI_BG_GATE_UP: {
            const BgEpiSwiGLU g{e.act, e.inter, e.act_mode, nullptr};
            return bg8o_launch(x, norm_w, eps, data, scales, tiled, K, B, g, g, p, workspace, s);
        }
        case SLI_BG_STORE: {
            const BgEpiStore y{e.y, e.resid, nullptr, e.scale, e.nrows, e.ld};
            return bg8o_launch(x, norm_w, eps, data, scales, tiled, K, B, y, y, p, workspace, s);
        }
        default: {
            const BgEpiLogits l{e.logits, (unsigned long long*)e.keys_out, e.nrows, e.ld, e.vocab_off, e.key_ld, nullptr};
            return bg8o_launch(x, norm_w, eps, data, scales, tiled, K, B, l, l, p, workspace, s);
        }
    }
}

}  // namespace sli

using namespace sli;

extern "C" {

int sli_quant_mxfp8(const float* src, void* codes, void* scales, int32_t rows, int32_t cols, sli_stream_t stream) {
    SLI_CHECK(src && codes && scales, SLI_ERR_ARG, "sli_quant_mxfp8: null pointer");
    SLI_CHECK(rows > 0 && cols > 0 && cols % kMxBlock == 0, SLI_ERR_SHAPE, "sli_quant_mxfp8: cols must be a multiple of 32");
    SLI_CHECK(mx8_al(src, 16) && mx8_al(codes, 4), SLI_ERR_ARG, "sli_quant_mxfp8: src needs 16-byte, codes 4-byte alignment");
    return mx8_quant_launch<Mx8SrcF32, false>(Mx8SrcF32{src}, nullptr, codes, scales, rows, cols, 0.0f, as_stream(stream));
}

int sli_dequant_mxfp8(const void* codes, const void* scales, float* dst, int32_t rows, int32_t cols, sli_stream_t stream) {
    SLI_CHECK(codes && scales && dst, SLI_ERR_ARG, "sli_dequant_mxfp8: null pointer");
    SLI_CHECK(rows > 0 && cols > 0 && cols % kMxBlock == 0, SLI_ERR_SHAPE, "sli_dequant_mxfp8: cols must be a multiple of 32");
    const size_t n = (size_t)rows * cols;
    hipLaunchKernelGGL(dequant_mx8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       (const uint8_t*)codes, (const uint8_t*)scales, dst, n);
    SLI_HIP(hipGetLastError());
    return SLI_OK;
}

int sli_prefill_norm_quant_mx8(const float* x, const float* w, void* codes, void* scales, int32_t M, int32_t D, float eps,
                               sli_stream_t stream) {
    SLI_CHECK(x && codes && scales, SLI_ERR_ARG, "sli_prefill_norm_quant_mx8: null pointer");
    SLI_CHECK(M >= 1 && M <= 65535, SLI_ERR_ARG, "sli_prefill_norm_quant_mx8: M must be in [1, 65535]");
    SLI_CHECK(D >= 32 && D % 32 == 0 && (!w || D <= 8192), SLI_ERR_ARG,
              "sli_prefill_norm_quant_mx8: D must be a multiple of 32, with norm weights at most 8192 (the row is held in "
              "registers)");
    SLI_CHECK(mx8_al(x, 16) && mx8_al(w, 16) && mx8_al(codes, 16), SLI_ERR_ARG, "sli_prefill_norm_quant_mx8: 16-byte alignment");
    return mx8_norm_quant(x, w, codes, scales, M, D, eps, as_stream(stream));
}

int sli_prefill_quant_mx8(const void* hi, const void* lo, void* codes, void* scales, int32_t M, int32_t D,
                          sli_stream_t stream) {
    SLI_CHECK(hi && lo && codes && scales, SLI_ERR_ARG, "sli_prefill_quant_mx8: null pointer");
    SLI_CHECK(M >= 1 && M <= 65535, SLI_ERR_ARG, "sli_prefill_quant_mx8: M must be in [1, 65535]");
    SLI_CHECK(D >= 32 && D % 32 == 0, SLI_ERR_ARG, "sli_prefill_quant_mx8: D must be a multiple of 32");
    SLI_CHECK(mx8_al(hi, 16) && mx8_al(lo, 16) && mx8_al(codes, 16), SLI_ERR_ARG, "sli_prefill_quant_mx8: 16-byte alignment");
    return mx8_pair_quant(hi, lo, codes, scales, M, D, as_stream(stream));
}

int sli_prefill_gemm_mx8(const void* data, const void* scales, const void* acodes, const void* ascales, int32_t N,
                         int32_t K, int32_t M, int32_t p0, int32_t nv, const sli_pgemm_epilogue* epi, void* state,
                         sli_pgemm_tiling* tiling, sli_stream_t stream) {
    SLI_CHECK(data && scales && acodes && ascales && epi && state, SLI_ERR_ARG, "sli_prefill_gemm_mx8: null pointer");
    bool chunk = false;
    for (int sz : kPfSizes) chunk = chunk || M == sz;
    SLI_CHECK(chunk, SLI_ERR_ARG, "sli_prefill_gemm_mx8: M must be 32, 64, 128 or 256");
    SLI_CHECK(K >= 128 && K % 128 == 0, SLI_ERR_SHAPE, "sli_prefill_gemm_mx8: K must be a multiple of 128 (one MFMA issue)");
    SLI_CHECK(N >= 16 && (N % 16 == 0 || epi->role == 3), SLI_ERR_ARG,
              "sli_prefill_gemm_mx8: N must be a multiple of 16 (role 3: at least 16)");
    SLI_CHECK((int64_t)N * K < ((int64_t)1 << 40) && K <= (1 << 20), SLI_ERR_ARG, "sli_prefill_gemm_mx8: shape too large");
    SLI_CHECK(mx8_al(data, 16) && mx8_al(acodes, 16) && mx8_al(scales, 4) && mx8_al(ascales, 4), SLI_ERR_ARG,
              "sli_prefill_gemm_mx8: data and acodes need 16-byte, scales and ascales 4-byte alignment");
    SLI_CHECK(p0 >= 0 && p0 <= (1 << 30) && nv >= 1 && nv <= M, SLI_ERR_ARG,
              "sli_prefill_gemm_mx8: p0 must be >= 0 and nv in [1, M]");
    SLI_CHECK(mx8_al(state, 8), SLI_ERR_ARG, "sli_prefill_gemm_mx8: state needs 8-byte alignment");
    const sli_pgemm_epilogue& e = *epi;
    switch (e.role) {
        case 0:
            SLI_CHECK(e.q && e.kc && e.vc && e.sin_t && e.cos_t, SLI_ERR_ARG, "sli_prefill_gemm_mx8: null q/k/v operand");
            SLI_CHECK(e.kv_dtype == SLI_DT_F16 || e.kv_dtype == SLI_DT_F32 || e.kv_dtype == SLI_DT_F8E4M3, SLI_ERR_ARG,
                      "sli_prefill_gemm_mx8: bad kv dtype");
            SLI_CHECK(e.hd == 64 || e.hd == 128, SLI_ERR_ARG, "sli_prefill_gemm_mx8: head_dim must be 64 or 128");
            SLI_CHECK(e.hq >= 1 && e.hkv >= 1 && e.hq % e.hkv == 0, SLI_ERR_ARG,
                      "sli_prefill_gemm_mx8: hq must be a multiple of hkv");
            SLI_CHECK((int64_t)N == ((int64_t)e.hq + 2 * (int64_t)e.hkv) * e.hd, SLI_ERR_ARG,
                      "sli_prefill_gemm_mx8: N must be (hq + 2 hkv) * hd");
            SLI_CHECK(e.T >= 1, SLI_ERR_ARG, "sli_prefill_gemm_mx8: T must be positive");
            SLI_CHECK(mx8_al(e.q, 16) && mx8_al(e.kc, 16) && mx8_al(e.vc, 16) && mx8_al(e.sin_t, 16) && mx8_al(e.cos_t, 16),
                      SLI_ERR_ARG, "sli_prefill_gemm_mx8: 16-byte alignment");
            break;
        case 1:
            SLI_CHECK(e.ahi && e.alo, SLI_ERR_ARG, "sli_prefill_gemm_mx8: null gate/up operand");
            SLI_CHECK(e.inter >= 8 && N == 2 * e.inter, SLI_ERR_ARG, "sli_prefill_gemm_mx8: N must be 2 * inter");
            SLI_CHECK(e.act_mode == 0 || e.act_mode == 1, SLI_ERR_ARG, "sli_prefill_gemm_mx8: act_mode must be 0 or 1");
            SLI_CHECK(mx8_al(e.ahi, 16) && mx8_al(e.alo, 16), SLI_ERR_ARG, "sli_prefill_gemm_mx8: 16-byte alignment");
            break;
        case 2:
        case 3:
            SLI_CHECK(e.y, SLI_ERR_ARG, "sli_prefill_gemm_mx8: null y");
            SLI_CHECK(e.ld >= N && e.ld % 4 == 0, SLI_ERR_ARG, "sli_prefill_gemm_mx8: ld must be >= N and a multiple of 4");
            SLI_CHECK(mx8_al(e.y, 16) && (e.role == 3 || mx8_al(e.resid, 16)), SLI_ERR_ARG,
                      "sli_prefill_gemm_mx8: 16-byte alignment");
            break;
        default:
            return fail(SLI_ERR_ARG, "sli_prefill_gemm_mx8: role must be 0 (qkv), 1 (gate/up), 2 (wo/down) or 3 (logits)");
    }
    hipStream_t s = as_stream(stream);
    if (int rc = mx8_prepare()) return rc;
    static_assert(sizeof(PfSegs) == 3 * 16 * sizeof(int32_t), "pg8_set_run_kernel: three arrays of 16 entries, a thread each");
    hipLaunchKernelGGL(pg8_set_run_kernel, dim3(1), dim3(sizeof(PfSegs) / 4), 0, s, (PfSegs*)state, p0, nv, M);
    SLI_HIP(hipGetLastError());
    return mx8_gemm(data, scales, acodes, ascales, N, K, M, e, state, tiling, s);
}

size_t sli_batch_gemm_mx8_workspace_bytes(int32_t rows, int32_t K, int32_t B, int32_t norm, int32_t tiled,
                                          sli_bgemm_mx8_plan* plan) {
    if (!plan) return 0;
    Bg8Plan p;
    if (const char* why = bg8o_plan(rows, K, B, norm != 0, plan, p)) {
        fail(SLI_ERR_SHAPE, std::string("sli_batch_gemm_mx8_workspace_bytes: ") + why);
        return 0;
    }
    return bg8o_ws_bytes(p, K, tiled);
}

int sli_batch_gemm_mx8(const float* x, const float* norm_w, float eps, const void* data, const void* scales, int32_t tiled,
                       int32_t K, int32_t B, const sli_bgemm_epilogue* epi, sli_bgemm_mx8_plan* plan, void* workspace,
                       size_t workspace_bytes, sli_stream_t stream) {
    const std::string fn = "sli_batch_gemm_mx8";
    SLI_CHECK(x && data && scales && epi && plan && workspace, SLI_ERR_ARG, fn + ": null pointer");
    SLI_CHECK(K >= kBg8Stage && K % kBg8Stage == 0, SLI_ERR_SHAPE, fn + ": K must be a positive multiple of 128 (one MFMA issue)");
    SLI_CHECK(B >= 1 && B <= kBgMaxBatch, SLI_ERR_SHAPE, fn + ": batch must be in [1, 8]");
    const sli_bgemm_epilogue& e = *epi;
    if (e.role == SLI_BG_QKV)
        SLI_CHECK(e.hq >= 1 && e.hkv >= 1 && e.hd >= 1 && bgo_epilogue_rows(e) % 16 == 0, SLI_ERR_SHAPE,
                  fn + ": (hq + 2 hkv) * hd must be a multiple of 16");
    if (e.role == SLI_BG_GATE_UP)
        SLI_CHECK(e.inter >= 8 && e.inter % 8 == 0, SLI_ERR_SHAPE, fn + ": inter must be a positive multiple of 8");
    SLI_CHECK(mx8_al(x, 16) && mx8_al(norm_w, 16) && mx8_al(data, 16) && mx8_al(scales, 16) && mx8_al(workspace, 16),
              SLI_ERR_ARG, fn + ": 16-byte alignment");
    const bool norm = norm_w != nullptr;
    if (int rc = bgo_check_epilogue(fn, e, norm)) return rc;
    Bg8Plan p;
    if (const char* why = bg8o_plan(bgo_epilogue_rows(e), K, B, norm, plan, p)) return fail(SLI_ERR_ARG, fn + ": " + why);
    SLI_CHECK(e.role != SLI_BG_LOGITS || e.key_ld >= p.groups, SLI_ERR_ARG, fn + ": key_ld must hold one key per workgroup group");
    SLI_CHECK(workspace_bytes >= bg8o_ws_bytes(p, K, tiled), SLI_ERR_ARG, fn + ": workspace too small");
    return bg8o_role(x, norm_w, eps, data, scales, tiled, K, B, e, p, workspace, as_stream(stream));
}

// The plain-rows projection: the store role with no residual and scale 1, the planner's plan, counters zeroed here
size_t sli_matmul_batch_mx8_workspace_bytes(int32_t rows, int32_t cols, int32_t batch, int32_t tiled) {
    sli_bgemm_mx8_plan io{};
    Bg8Plan p;
    if (bg8o_plan(rows, cols, batch, false, &io, p)) return 0;
    return bg8o_ws_bytes(p, cols, tiled);
}

int sli_matmul_batch_mx8(const float* x, const void* data, const void* scales, float* y, int32_t rows, int32_t cols,
                         int32_t batch, int32_t tiled, void* workspace, size_t workspace_bytes, sli_stream_t stream) {
    SLI_CHECK(x && data && scales && y && workspace, SLI_ERR_ARG, "sli_matmul_batch_mx8: null pointer");
    SLI_CHECK(rows > 0 && cols >= kBg8Stage && cols % kBg8Stage == 0, SLI_ERR_SHAPE,
              "sli_matmul_batch_mx8: cols must be a positive multiple of 128 (one MFMA issue)");
    SLI_CHECK(batch >= 1 && batch <= kBgMaxBatch, SLI_ERR_SHAPE, "sli_matmul_batch_mx8: batch must be in [1, 8]");
    SLI_CHECK(mx8_al(x, 16) && mx8_al(data, 16) && mx8_al(scales, 16) && mx8_al(y, 16) && mx8_al(workspace, 16), SLI_ERR_ARG,
              "sli_matmul_batch_mx8: 16-byte alignment");
    sli_bgemm_mx8_plan io{};
    Bg8Plan p;
    if (const char* why = bg8o_plan(rows, cols, batch, false, &io, p)) return fail(SLI_ERR_SHAPE, std::string("sli_matmul_batch_mx8: ") + why);
    SLI_CHECK(workspace_bytes >= bg8o_ws_bytes(p, cols, tiled), SLI_ERR_ARG, "sli_matmul_batch_mx8: workspace too small");
    hipStream_t s = as_stream(stream);
    SLI_HIP(hipMemsetAsync((char*)workspace + bg8_part_bytes(p), 0, sizeof(unsigned) * p.groups, s));
    const BgEpiStore e{y, nullptr, nullptr, 1.0f, rows, rows};
    return bg8o_launch(x, nullptr, 0.0f, data, scales, tiled, cols, batch, e, e, p, workspace, s);
}

}  // extern "C"
