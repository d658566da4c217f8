// i8a8.hip — the per-token int8 activation image and the integer-MFMA prefill GEMM (pgemm_i8a8.h) as entry points of the
// C ABI (include/sli.h): the two quantising producers and one GEMM launch. A translation unit of its own: it holds the
// one compiled copy of every pgemm_i8a8 kernel.
#include "i8a8_api.h"
#include "pgemm_i8a8.h"

namespace sli {

static bool i8a8_al(const void* p, uintptr_t a) { return (uintptr_t)p % a == 0; }

template <class Src, bool NORM>
static int i8a8_quant_launch(const Src& src, const float* w, void* codes, float* scales, int rows, int D, float eps,
                             hipStream_t s) {
    hipLaunchKernelGGL((pf_quant_i8_kernel<Src, NORM>), dim3(rows), dim3(256), 0, s, src, w, (int8_t*)codes, scales, D, eps);
    SLI_HIP(hipGetLastError());
    return SLI_OK;
}

template <class Epi>
static int i8a8_gemm_launch(const PgI8A8In& in, int role, const Epi& e, sli_pgemm_tiling* tiling, hipStream_t s) {
    return pg_i8a8_pick(in.M, role, [&](auto cfg) -> int {
        using Cfg = decltype(cfg);
        if (tiling) *tiling = sli_pgemm_tiling{Cfg::BM, Cfg::WR, Cfg::S, Cfg::AT, 1, 0, PgI8A8Geo<Cfg>::KS};
        SLI_HIP((launch_pgemm_i8a8<Epi, Cfg>(in, e, s)));
        return SLI_OK;
    });
}

int i8a8_prepare() {
    static const hipError_t err = [] {
        hipError_t e = pg_i8a8_allow_lds_all<PgEpiQKV<f8e4m3>>();
        if (e == hipSuccess) e = pg_i8a8_allow_lds_all<PgEpiQKV<__half>>();
        if (e == hipSuccess) e = pg_i8a8_allow_lds_all<PgEpiQKV<float>>();
        if (e == hipSuccess) e = pg_i8a8_allow_lds_all<PgEpiSwiGLU>();
        if (e == hipSuccess) e = pg_i8a8_allow_lds_all<PgEpiResid>();
        if (e == hipSuccess) e = pg_i8a8_allow_lds_all<PgEpiLogits>();
        return e;
    }();
    SLI_HIP(err);
    return SLI_OK;
}
int i8a8_norm_quant(const float* x, const float* w, void* codes, float* scales, int M, int D, float eps, hipStream_t s) {
    const Mx8SrcF32 src{x};
    if (w) return i8a8_quant_launch<Mx8SrcF32, true>(src, w, codes, scales, M, D, eps, s);
    return i8a8_quant_launch<Mx8SrcF32, false>(src, nullptr, codes, scales, M, D, eps, s);
}
int i8a8_pair_quant(const void* hi, const void* lo, void* codes, float* scales, int M, int D, hipStream_t s) {
    const Mx8SrcPair src{(const __half*)hi, (const __half*)lo};
    return i8a8_quant_launch<Mx8SrcPair, false>(src, nullptr, codes, scales, M, D, 0.0f, s);
}
int i8a8_gemm(const void* w, const float* rs, const void* acodes, const float* ascales, int N, int K, int M,
              const sli_pgemm_epilogue& e, const void* segs_, sli_pgemm_tiling* tiling, hipStream_t s) {
    const PgI8A8In in{(const int8_t*)w, (const int8_t*)acodes, ascales, N, K, M};
    const PfSegs* segs = (const PfSegs*)segs_;
    if (e.role == 0) {
        if (e.kv_dtype == SLI_DT_F8E4M3) {
            const PgEpiQKV<f8e4m3> q{e.q, (f8e4m3*)e.kc, (f8e4m3*)e.vc, rs, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T, segs};
            return i8a8_gemm_launch(in, 0, q, tiling, s);
        }
        if (e.kv_dtype == SLI_DT_F16) {
            const PgEpiQKV<__half> q{e.q, (__half*)e.kc, (__half*)e.vc, rs, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T, segs};
            return i8a8_gemm_launch(in, 0, q, tiling, s);
        }
        const PgEpiQKV<float> q{e.q, (float*)e.kc, (float*)e.vc, rs, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T, segs};
        return i8a8_gemm_launch(in, 0, q, tiling, s);
    }
    if (e.role == 1) {
        const PgEpiSwiGLU g{(__half*)e.ahi, (__half*)e.alo, rs, e.inter, e.act_mode};
        return i8a8_gemm_launch(in, 1, g, tiling, s);
    }
    if (e.role == 3) {  // any N >= 16: the launch covers whole 16-row tiles, the epilogue masks at N
        const PgEpiLogits g{e.y, rs, in.N, e.ld};
        PgI8A8In up = in;
        up.N = pg_logits_n(in.N);
        return i8a8_gemm_launch(up, 3, g, tiling, s);
    }
    const PgEpiResid r{e.y, e.resid, rs, in.N, e.ld};
    return i8a8_gemm_launch(in, 2, r, tiling, s);
}

}  // namespace sli

using namespace sli;

extern "C" {

int sli_prefill_norm_quant_i8(const float* x, const float* w, void* codes, float* scales, int32_t M, int32_t D, float eps,
                              sli_stream_t stream) {
    SLI_CHECK(x && codes && scales, SLI_ERR_ARG, "sli_prefill_norm_quant_i8: null pointer");
    SLI_CHECK(M >= 1 && M <= 65535, SLI_ERR_ARG, "sli_prefill_norm_quant_i8: M must be in [1, 65535]");
    SLI_CHECK(D >= 4 && D % 4 == 0 && (!w || D <= 8192), SLI_ERR_ARG,
              "sli_prefill_norm_quant_i8: D must be a multiple of 4, with norm weights at most 8192 (the row is held in "
              "registers)");
    SLI_CHECK(i8a8_al(x, 16) && i8a8_al(w, 16) && i8a8_al(codes, 16) && i8a8_al(scales, 4), SLI_ERR_ARG,
              "sli_prefill_norm_quant_i8: x, w and codes need 16-byte, scales 4-byte alignment");
    return i8a8_norm_quant(x, w, codes, scales, M, D, eps, as_stream(stream));
}

int sli_prefill_quant_i8(const void* hi, const void* lo, void* codes, float* scales, int32_t M, int32_t D,
                         sli_stream_t stream) {
    SLI_CHECK(hi && lo && codes && scales, SLI_ERR_ARG, "sli_prefill_quant_i8: null pointer");
    SLI_CHECK(M >= 1 && M <= 65535, SLI_ERR_ARG, "sli_prefill_quant_i8: M must be in [1, 65535]");
    SLI_CHECK(D >= 4 && D % 4 == 0, SLI_ERR_ARG, "sli_prefill_quant_i8: D must be a multiple of 4");
    SLI_CHECK(i8a8_al(hi, 16) && i8a8_al(lo, 16) && i8a8_al(codes, 16) && i8a8_al(scales, 4), SLI_ERR_ARG,
              "sli_prefill_quant_i8: hi, lo and codes need 16-byte, scales 4-byte alignment");
    return i8a8_pair_quant(hi, lo, codes, scales, M, D, as_stream(stream));
}

int sli_prefill_gemm_i8a8(const void* w, const float* w_row_scale, const void* acodes, const float* ascales, int32_t N,
                          int32_t K, int32_t M, int32_t p0, int32_t nv, const sli_pgemm_epilogue* epi, void* state,
                          sli_pgemm_tiling* tiling, sli_stream_t stream) {
    SLI_CHECK(w && acodes && ascales && epi && state, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: null pointer");
    bool chunk = false;
    for (int sz : kPfSizes) chunk = chunk || M == sz;
    SLI_CHECK(chunk, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: M must be 32, 64, 128 or 256");
    SLI_CHECK(K >= 128 && K % 128 == 0, SLI_ERR_SHAPE, "sli_prefill_gemm_i8a8: K must be a multiple of 128 (one stage)");
    SLI_CHECK(K <= kI8A8MaxK, SLI_ERR_SHAPE, "sli_prefill_gemm_i8a8: K must be at most 131072 (the i32 accumulator)");
    SLI_CHECK(N >= 16 && (N % 16 == 0 || epi->role == 3), SLI_ERR_ARG,
              "sli_prefill_gemm_i8a8: N must be a multiple of 16 (role 3: at least 16)");
    SLI_CHECK((int64_t)N * K < ((int64_t)1 << 40), SLI_ERR_ARG, "sli_prefill_gemm_i8a8: shape too large");
    SLI_CHECK(i8a8_al(w, 16) && i8a8_al(acodes, 16) && i8a8_al(w_row_scale, 16) && i8a8_al(ascales, 4), SLI_ERR_ARG,
              "sli_prefill_gemm_i8a8: w, acodes and w_row_scale need 16-byte, ascales 4-byte alignment");
    SLI_CHECK(p0 >= 0 && p0 <= (1 << 30) && nv >= 1 && nv <= M, SLI_ERR_ARG,
              "sli_prefill_gemm_i8a8: p0 must be >= 0 and nv in [1, M]");
    SLI_CHECK(i8a8_al(state, 8), SLI_ERR_ARG, "sli_prefill_gemm_i8a8: state needs 8-byte alignment");
    const sli_pgemm_epilogue& e = *epi;
    switch (e.role) {
        case 0:
            SLI_CHECK(e.q && e.kc && e.vc && e.sin_t && e.cos_t, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: null q/k/v operand");
            SLI_CHECK(e.kv_dtype == SLI_DT_F16 || e.kv_dtype == SLI_DT_F32 || e.kv_dtype == SLI_DT_F8E4M3, SLI_ERR_ARG,
                      "sli_prefill_gemm_i8a8: bad kv dtype");
            SLI_CHECK(e.hd == 64 || e.hd == 128, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: head_dim must be 64 or 128");
            SLI_CHECK(e.hq >= 1 && e.hkv >= 1 && e.hq % e.hkv == 0, SLI_ERR_ARG,
                      "sli_prefill_gemm_i8a8: hq must be a multiple of hkv");
            SLI_CHECK((int64_t)N == ((int64_t)e.hq + 2 * (int64_t)e.hkv) * e.hd, SLI_ERR_ARG,
                      "sli_prefill_gemm_i8a8: N must be (hq + 2 hkv) * hd");
            SLI_CHECK(e.T >= 1, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: T must be positive");
            SLI_CHECK(i8a8_al(e.q, 16) && i8a8_al(e.kc, 16) && i8a8_al(e.vc, 16) && i8a8_al(e.sin_t, 16) && i8a8_al(e.cos_t, 16),
                      SLI_ERR_ARG, "sli_prefill_gemm_i8a8: 16-byte alignment");
            break;
        case 1:
            SLI_CHECK(e.ahi && e.alo, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: null gate/up operand");
            SLI_CHECK(e.inter >= 8 && N == 2 * e.inter, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: N must be 2 * inter");
            SLI_CHECK(e.act_mode == 0 || e.act_mode == 1, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: act_mode must be 0 or 1");
            SLI_CHECK(i8a8_al(e.ahi, 16) && i8a8_al(e.alo, 16), SLI_ERR_ARG, "sli_prefill_gemm_i8a8: 16-byte alignment");
            break;
        case 2:
        case 3:
            SLI_CHECK(e.y, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: null y");
            SLI_CHECK(e.ld >= N && e.ld % 4 == 0, SLI_ERR_ARG, "sli_prefill_gemm_i8a8: ld must be >= N and a multiple of 4");
            SLI_CHECK(i8a8_al(e.y, 16) && (e.role == 3 || i8a8_al(e.resid, 16)), SLI_ERR_ARG,
                      "sli_prefill_gemm_i8a8: 16-byte alignment");
            break;
        default:
            return fail(SLI_ERR_ARG, "sli_prefill_gemm_i8a8: role must be 0 (qkv), 1 (gate/up), 2 (wo/down) or 3 (logits)");
    }
    hipStream_t s = as_stream(stream);
    if (int rc = i8a8_prepare()) return rc;
    static_assert(sizeof(PfSegs) == 3 * 16 * sizeof(int32_t), "pg8_set_run_kernel: three arrays of 16 entries, a thread each");
    hipLaunchKernelGGL(pg8_set_run_kernel, dim3(1), dim3(sizeof(PfSegs) / 4), 0, s, (PfSegs*)state, p0, nv, M);
    SLI_HIP(hipGetLastError());
    return i8a8_gemm(w, w_row_scale, acodes, ascales, N, K, M, e, state, tiling, s);
}

}  // extern "C"
