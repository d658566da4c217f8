// prefill_ops.h — the prefill stages as kernel-level entry points (include/sli.h "prefill stages, for tests and
// labs"): one launch of pf_norm_split_kernel, pgemm_kernel or a prefill attention kernel on caller-provided device
// buffers. Included once, at the end of engine.hip, so the library holds ONE compiled copy of every prefill kernel:
// the entries launch the very code objects sli_model_prefill launches. The GEMM tiling comes from prefill.h pg_pick
// and the attention kernel from launch_pf_attn, the functions the engine's record_pf_phase uses. The checks mirror
// the engine's pf_supported and the contracts stated in prefill.h: whatever a kernel would read or write out of
// bounds for is refused here.
#pragma once
#include <cmath>

#include "common.h"
#include "prefill.h"
#include "score.h"

namespace sli {

static_assert(sizeof(PfSegs) == SLI_PF_TABLE_BYTES, "sli.h states the table's size");

// the group table of a chunk (prefill.h PfSegs), written on the stream: one dword per thread
__global__ void pf_set_segs_kernel(PfSegs* dst, PfSegs v) {
    reinterpret_cast<int32_t*>(dst)[threadIdx.x] = reinterpret_cast<const int32_t*>(&v)[threadIdx.x];
}

static int pf_put_segs(void* table, const PfSegs& v, hipStream_t s) {
    hipLaunchKernelGGL(pf_set_segs_kernel, dim3(1), dim3(sizeof(PfSegs) / 4), 0, s, (PfSegs*)table, v);
    SLI_HIP(hipGetLastError());
    return SLI_OK;
}

// the plain entries' table: M rows of one sequence from p0 on, the first nv valid (any p0: the kernels need no
// alignment, only the packed route's bit-equality argument does)
static int pf_set_run(void* table, int p0, int nv, int M, hipStream_t s) {
    PfSegs v{};
    for (int g = 0; g < M / 16; ++g) {
        v.p0[g] = p0 + 16 * g;
        v.nv[g] = std::min(std::max(nv - 16 * g, 0), 16);
    }
    return pf_put_segs(table, v, s);
}

// groups: M / 16 host entries; the table's other entries are padding groups
static int pf_set_segs(void* table, const sli_pf_group* groups, int M, int B, int T, hipStream_t s) {
    SLI_CHECK(groups && table && (uintptr_t)table % 4 == 0, SLI_ERR_ARG, "prefill segs: null or misaligned group table");
    SLI_CHECK(B >= 1 && T >= 1, SLI_ERR_ARG, "prefill segs: B and T must be positive");
    PfSegs v{};
    for (int g = 0; g < M / 16; ++g) {
        const sli_pf_group& gr = groups[g];
        SLI_CHECK(gr.seq >= 0 && gr.seq < B, SLI_ERR_ARG, "prefill segs: a group's sequence must be in [0, B)");
        SLI_CHECK(gr.p0 >= 0 && gr.p0 < T && gr.p0 % 16 == 0, SLI_ERR_ARG,
                  "prefill segs: a group's p0 must be a multiple of 16 in [0, T)");
        SLI_CHECK(gr.nv >= 0 && gr.nv <= 16, SLI_ERR_ARG, "prefill segs: a group's nv must be in [0, 16]");
        v.seq[g] = gr.seq;
        v.p0[g] = gr.p0;
        v.nv[g] = gr.nv;
    }
    return pf_put_segs(table, v, s);
}

static bool pf_chunk_size(int M) {
    for (int s : kPfSizes)
        if (M == s) return true;
    return false;
}

static bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }

template <class Epi, typename WT>
static int pf_gemm_launch(const void* w, const void* ws, const void* hi, const void* lo, int N, int K, int M, int role, const Epi& e,
                          sli_pgemm_tiling* tiling, hipStream_t s) {
    SLI_HIP((pg_allow_lds_all<Epi, WT>()));
    return pg_pick<WT>(M, role, [&](auto cfg) -> int {
        using Cfg = decltype(cfg);
        if (tiling)
            *tiling = sli_pgemm_tiling{Cfg::BM, Cfg::WR, Cfg::S, Cfg::AT, Cfg::PIPE ? 1 : 0, Cfg::SA, PgGeo<Cfg, WT>::KS};
        // ws: the e8m0 block scales (mxfp4), else null
        const PgIn<WT> in{(const WT*)w, (const __half*)hi, (const __half*)lo, N, K, M, (const uint8_t*)ws};
        SLI_HIP((launch_pgemm<Epi, Cfg, WT>(in, e, s)));
        return SLI_OK;
    });
}

// rs: int8 row scales for the epilogue (nullable); mxfp4: ws, the block scales for the GEMM, and no row scale. segs:
// the chunk's table on the device (read by role 0 alone)
template <typename WT>
static int pf_gemm_role(const void* w, const float* rs_in, const void* hi, const void* lo, int N, int K, int M,
                        const sli_pgemm_epilogue& e, const PfSegs* segs, sli_pgemm_tiling* tiling, hipStream_t s) {
    const void* ws = is_mx<WT>::value ? (const void*)rs_in : nullptr;
    const float* rs = is_mx<WT>::value ? nullptr : rs_in;
    if (e.role == 0) {
        if (e.kv_dtype == SLI_DT_F8E4M3) {
            const PgEpiQKV<f8e4m3> q{e.q, (f8e4m3*)e.kc, (f8e4m3*)e.vc, rs, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T, segs};
            return pf_gemm_launch<PgEpiQKV<f8e4m3>, WT>(w, ws, hi, lo, N, K, M, 0, q, tiling, s);
        }
        if (e.kv_dtype == SLI_DT_F16) {
            const PgEpiQKV<__half> q{e.q, (__half*)e.kc, (__half*)e.vc, rs, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T, segs};
            return pf_gemm_launch<PgEpiQKV<__half>, WT>(w, ws, hi, lo, N, K, M, 0, q, tiling, s);
        }
        const PgEpiQKV<float> q{e.q, (float*)e.kc, (float*)e.vc, rs, e.sin_t, e.cos_t, e.hq, e.hkv, e.hd, e.T, segs};
        return pf_gemm_launch<PgEpiQKV<float>, WT>(w, ws, hi, lo, N, K, M, 0, q, tiling, s);
    }
    if (e.role == 1) {
        const PgEpiSwiGLU g{(__half*)e.ahi, (__half*)e.alo, rs, e.inter, e.act_mode};
        return pf_gemm_launch<PgEpiSwiGLU, WT>(w, ws, hi, lo, N, K, M, 1, g, tiling, s);
    }
    if (e.role == 3) {  // N weight rows, any N >= 16: the launch covers whole 16-row tiles, the epilogue masks at N
        const PgEpiLogits g{e.y, rs, N, e.ld};
        return pf_gemm_launch<PgEpiLogits, WT>(w, ws, hi, lo, pg_logits_n(N), K, M, 3, g, tiling, s);
    }
    const PgEpiResid r{e.y, e.resid, rs, N, e.ld};
    return pf_gemm_launch<PgEpiResid, WT>(w, ws, hi, lo, N, K, M, 2, r, tiling, s);
}

// one pgemm_kernel launch under the table the entry has just put on the stream; ws: mxfp4 block scales or int8 row scales
static int pf_gemm_run(const void* w, int w_dtype, const void* ws, const void* hi, const void* lo, int N, int K, int M,
                       const sli_pgemm_epilogue& e, const void* table, sli_pgemm_tiling* tiling, hipStream_t s) {
    const PfSegs* segs = (const PfSegs*)table;
    const float* rs = (const float*)ws;
    if (w_dtype == SLI_DT_MXFP4) return pf_gemm_role<mxfp4>(w, rs, hi, lo, N, K, M, e, segs, tiling, s);
    if (w_dtype == SLI_DT_I8) return pf_gemm_role<int8_t>(w, rs, hi, lo, N, K, M, e, segs, tiling, s);
    return pf_gemm_role<__half>(w, rs, hi, lo, N, K, M, e, segs, tiling, s);
}

// one attention launch under the table the entry has just put on the stream (an fp32 cache: the one-sequence kernel)
static int pf_attn_run(const float* q, const void* kc, const void* vc, int kv_dtype, void* ohi, void* olo, int M, int hq,
                       int hkv, int hd, int T, const void* table, hipStream_t s) {
    const PfSegs* segs = (const PfSegs*)table;
    const float scale = 1.0f / sqrtf((float)hd);
    if (kv_dtype == SLI_DT_F16) {
        const PfAttnArgs<__half> aa{q, (const __half*)kc, (const __half*)vc, (__half*)ohi, (__half*)olo, hq, hkv, T, scale};
        SLI_HIP(launch_pf_attn<__half>(aa, hd, M, segs, s));
    } else if (kv_dtype == SLI_DT_F8E4M3) {  // every DMA piece is 16 bytes of a row: the entries' al16 check
        const PfAttnArgs<f8e4m3> aa{q, (const f8e4m3*)kc, (const f8e4m3*)vc, (__half*)ohi, (__half*)olo, hq, hkv, T, scale};
        SLI_HIP(launch_pf_attn<f8e4m3>(aa, hd, M, segs, s));
    } else {
        const PfAttnArgs<float> aa{q, (const float*)kc, (const float*)vc, (__half*)ohi, (__half*)olo, hq, hkv, T, scale};
        SLI_HIP(launch_pf_attn<float>(aa, hd, M, segs, s));
    }
    return SLI_OK;
}

}  // namespace sli

using namespace sli;

extern "C" {

int sli_prefill_norm_split(const float* x, const float* w, void* hi, void* lo, int32_t M, int32_t D, float eps,
                           sli_stream_t stream) {
    SLI_CHECK(x && hi && lo, SLI_ERR_ARG, "sli_prefill_norm_split: null pointer");
    SLI_CHECK(M >= 1 && M <= 65535, SLI_ERR_ARG, "sli_prefill_norm_split: M must be in [1, 65535]");
    SLI_CHECK(D >= 4 && D % 4 == 0 && D <= 8192, SLI_ERR_ARG,
              "sli_prefill_norm_split: D must be a multiple of 4, at most 8192 (the row is held in registers)");
    SLI_CHECK(al16(x) && al16(w) && al16(hi) && al16(lo), SLI_ERR_ARG, "sli_prefill_norm_split: 16-byte alignment");
    hipLaunchKernelGGL(pf_norm_split_kernel, dim3(M), dim3(256), 0, as_stream(stream), x, w, (__half*)hi, (__half*)lo,
                       D, eps);
    SLI_HIP(hipGetLastError());
    return SLI_OK;
}

// the checks every GEMM entry shares (the plain and the group-table forms); ws: mxfp4 block scales (w_dtype
// SLI_DT_MXFP4) or int8 row scales
static int pf_gemm_check(const void* w, int w_dtype, const void* ws, const void* hi, const void* lo, int32_t N, int32_t K,
                         int32_t M, const sli_pgemm_epilogue* epi) {
    SLI_CHECK(pf_chunk_size(M), SLI_ERR_ARG, "sli_prefill_gemm: M must be 32, 64, 128 or 256");
    SLI_CHECK(K >= 64 && K % 64 == 0, SLI_ERR_ARG, "sli_prefill_gemm: K must be a multiple of 64");
    SLI_CHECK(N >= 16 && (N % 16 == 0 || epi->role == 3), SLI_ERR_ARG,
              "sli_prefill_gemm: N must be a multiple of 16 (role 3: at least 16)");
    SLI_CHECK((int64_t)N * K < ((int64_t)1 << 40) && K <= (1 << 20), SLI_ERR_ARG, "sli_prefill_gemm: shape too large");
    SLI_CHECK(al16(w) && (w_dtype == SLI_DT_MXFP4 || al16(ws)) && al16(hi) && al16(lo), SLI_ERR_ARG,
              "sli_prefill_gemm: 16-byte alignment");
    const sli_pgemm_epilogue& e = *epi;
    switch (e.role) {
        case 0:
            SLI_CHECK(e.q && e.kc && e.vc && e.sin_t && e.cos_t, SLI_ERR_ARG, "sli_prefill_gemm: null q/k/v operand");
            SLI_CHECK(e.kv_dtype == SLI_DT_F16 || e.kv_dtype == SLI_DT_F32 || e.kv_dtype == SLI_DT_F8E4M3, SLI_ERR_ARG,
                      "sli_prefill_gemm: bad kv dtype");
            SLI_CHECK(e.hd == 64 || e.hd == 128, SLI_ERR_ARG, "sli_prefill_gemm: head_dim must be 64 or 128");
            SLI_CHECK(e.hq >= 1 && e.hkv >= 1 && e.hq % e.hkv == 0, SLI_ERR_ARG,
                      "sli_prefill_gemm: hq must be a multiple of hkv");
            SLI_CHECK((int64_t)N == ((int64_t)e.hq + 2 * (int64_t)e.hkv) * e.hd, SLI_ERR_ARG,
                      "sli_prefill_gemm: N must be (hq + 2 hkv) * hd");
            SLI_CHECK(e.T >= 1, SLI_ERR_ARG, "sli_prefill_gemm: T must be positive");
            SLI_CHECK(al16(e.q) && al16(e.kc) && al16(e.vc) && al16(e.sin_t) && al16(e.cos_t), SLI_ERR_ARG,
                      "sli_prefill_gemm: 16-byte alignment");
            break;
        case 1:
            SLI_CHECK(e.ahi && e.alo, SLI_ERR_ARG, "sli_prefill_gemm: null gate/up operand");
            SLI_CHECK(e.inter >= 8 && N == 2 * e.inter, SLI_ERR_ARG, "sli_prefill_gemm: N must be 2 * inter");
            SLI_CHECK(e.act_mode == 0 || e.act_mode == 1, SLI_ERR_ARG, "sli_prefill_gemm: act_mode must be 0 or 1");
            SLI_CHECK(al16(e.ahi) && al16(e.alo), SLI_ERR_ARG, "sli_prefill_gemm: 16-byte alignment");
            break;
        case 2:
            SLI_CHECK(e.y, SLI_ERR_ARG, "sli_prefill_gemm: null y");
            SLI_CHECK(e.ld >= N && e.ld % 4 == 0, SLI_ERR_ARG, "sli_prefill_gemm: ld must be >= N and a multiple of 4");
            SLI_CHECK(al16(e.y) && al16(e.resid), SLI_ERR_ARG, "sli_prefill_gemm: 16-byte alignment");
            break;
        case 3:
            SLI_CHECK(e.y, SLI_ERR_ARG, "sli_prefill_gemm: null y");
            SLI_CHECK(e.ld >= N && e.ld % 4 == 0, SLI_ERR_ARG, "sli_prefill_gemm: ld must be >= N and a multiple of 4");
            SLI_CHECK(al16(e.y), SLI_ERR_ARG, "sli_prefill_gemm: 16-byte alignment");
            break;
        default:
            return fail(SLI_ERR_ARG, "sli_prefill_gemm: role must be 0 (qkv), 1 (gate/up), 2 (wo/down) or 3 (logits)");
    }
    return SLI_OK;
}

// the checks of both plain GEMM entries, their table and the launch
static int pf_gemm_entry(const void* w, int w_dtype, const void* ws, const void* hi, const void* lo, int32_t N, int32_t K,
                         int32_t M, int32_t p0, int32_t nv, const sli_pgemm_epilogue* epi, void* state,
                         sli_pgemm_tiling* tiling, sli_stream_t stream) {
    if (int rc = pf_gemm_check(w, w_dtype, ws, hi, lo, N, K, M, epi)) return rc;
    SLI_CHECK(p0 >= 0 && p0 <= (1 << 30) && nv >= 1 && nv <= M, SLI_ERR_ARG,
              "sli_prefill_gemm: p0 must be >= 0 and nv in [1, M]");
    SLI_CHECK((uintptr_t)state % 8 == 0, SLI_ERR_ARG, "sli_prefill_gemm: 16-byte alignment");
    hipStream_t s = as_stream(stream);
    if (int rc = pf_set_run(state, p0, nv, M, s)) return rc;
    return pf_gemm_run(w, w_dtype, ws, hi, lo, N, K, M, *epi, state, tiling, s);
}

int sli_prefill_gemm(const void* w, int w_dtype, const float* w_row_scale, const void* hi, const void* lo, int32_t N,
                     int32_t K, int32_t M, int32_t p0, int32_t nv, const sli_pgemm_epilogue* epi, void* state,
                     sli_pgemm_tiling* tiling, sli_stream_t stream) {
    SLI_CHECK(w && hi && lo && epi && state, SLI_ERR_ARG, "sli_prefill_gemm: null pointer");
    SLI_CHECK(w_dtype == SLI_DT_F16 || w_dtype == SLI_DT_I8, SLI_ERR_ARG,
              "sli_prefill_gemm: fp16 or int8 weights (fp32 and MXFP4 have no GEMM prefill)");
    return pf_gemm_entry(w, w_dtype, w_row_scale, hi, lo, N, K, M, p0, nv, epi, state, tiling, stream);
}

int sli_prefill_gemm_mxfp4(const void* data, const void* scales, const void* hi, const void* lo, int32_t N, int32_t K,
                           int32_t M, int32_t p0, int32_t nv, const sli_pgemm_epilogue* epi, void* state,
                           sli_pgemm_tiling* tiling, sli_stream_t stream) {
    SLI_CHECK(data && scales && hi && lo && epi && state, SLI_ERR_ARG, "sli_prefill_gemm_mxfp4: null pointer");
    return pf_gemm_entry(data, SLI_DT_MXFP4, scales, hi, lo, N, K, M, p0, nv, epi, state, tiling, stream);
}

int sli_prefill_attn(const float* q, const void* kc, const void* vc, int kv_dtype, void* ohi, void* olo, int32_t M,
                     int32_t rows_allocated, int32_t p0, int32_t hq, int32_t hkv, int32_t hd, int32_t T, void* state,
                     sli_stream_t stream) {
    SLI_CHECK(q && kc && vc && ohi && olo && state, SLI_ERR_ARG, "sli_prefill_attn: null pointer");
    SLI_CHECK(kv_dtype == SLI_DT_F16 || kv_dtype == SLI_DT_F32 || kv_dtype == SLI_DT_F8E4M3, SLI_ERR_ARG,
              "sli_prefill_attn: bad kv dtype");
    SLI_CHECK(pf_chunk_size(M), SLI_ERR_ARG, "sli_prefill_attn: M must be 32, 64, 128 or 256");
    SLI_CHECK(hd == 64 || hd == 128, SLI_ERR_ARG, "sli_prefill_attn: head_dim must be 64 or 128");
    SLI_CHECK(hq >= 1 && hkv >= 1 && hq % hkv == 0 && hq <= 65535, SLI_ERR_ARG,
              "sli_prefill_attn: hq must be a multiple of hkv");
    SLI_CHECK(T >= 1 && p0 >= 0 && p0 < T, SLI_ERR_ARG, "sli_prefill_attn: p0 must be in [0, T)");
    SLI_CHECK(rows_allocated >= pf_attn_rows(kv_dtype != SLI_DT_F32, M), SLI_ERR_ARG,
              "sli_prefill_attn: q / ohi / olo must hold M rows (fp32 cache: M rounded up to 64, the kernel's block)");
    SLI_CHECK(al16(q) && al16(kc) && al16(vc) && al16(ohi) && al16(olo) && (uintptr_t)state % 8 == 0, SLI_ERR_ARG,
              "sli_prefill_attn: 16-byte alignment");
    hipStream_t s = as_stream(stream);
    if (int rc = pf_set_run(state, p0, M, M, s)) return rc;
    return pf_attn_run(q, kc, vc, kv_dtype, ohi, olo, M, hq, hkv, hd, T, state, s);
}

// ---- the group-table forms (sli_model_prefill_seqs)
static int pf_gemm_qkv_segs_entry(const void* w, int w_dtype, const void* ws, const void* hi, const void* lo, int32_t N,
                                  int32_t K, int32_t M, const sli_pf_group* groups, int32_t B,
                                  const sli_pgemm_epilogue* epi, void* table, sli_pgemm_tiling* tiling,
                                  sli_stream_t stream) {
    SLI_CHECK(epi->role == 0, SLI_ERR_ARG, "sli_prefill_gemm_qkv_segs: the q/k/v epilogue (role 0) only");
    if (int rc = pf_gemm_check(w, w_dtype, ws, hi, lo, N, K, M, epi)) return rc;
    SLI_CHECK(epi->kv_dtype != SLI_DT_F32, SLI_ERR_ARG, "sli_prefill_gemm_qkv_segs: an fp16 or FP8 cache (fp32 has no table form)");
    hipStream_t s = as_stream(stream);
    if (int rc = pf_set_segs(table, groups, M, B, epi->T, s)) return rc;
    return pf_gemm_run(w, w_dtype, ws, hi, lo, N, K, M, *epi, table, tiling, s);
}

int sli_prefill_gemm_qkv_segs(const void* w, int w_dtype, const float* w_row_scale, const void* hi, const void* lo,
                              int32_t N, int32_t K, int32_t M, const sli_pf_group* groups, int32_t B,
                              const sli_pgemm_epilogue* epi, void* table, sli_pgemm_tiling* tiling, sli_stream_t stream) {
    SLI_CHECK(w && hi && lo && epi && groups && table, SLI_ERR_ARG, "sli_prefill_gemm_qkv_segs: null pointer");
    SLI_CHECK(w_dtype == SLI_DT_F16 || w_dtype == SLI_DT_I8, SLI_ERR_ARG,
              "sli_prefill_gemm_qkv_segs: fp16 or int8 weights (MXFP4: sli_prefill_gemm_qkv_segs_mxfp4)");
    return pf_gemm_qkv_segs_entry(w, w_dtype, w_row_scale, hi, lo, N, K, M, groups, B, epi, table, tiling, stream);
}

int sli_prefill_gemm_qkv_segs_mxfp4(const void* data, const void* scales, const void* hi, const void* lo, int32_t N,
                                    int32_t K, int32_t M, const sli_pf_group* groups, int32_t B,
                                    const sli_pgemm_epilogue* epi, void* table, sli_pgemm_tiling* tiling,
                                    sli_stream_t stream) {
    SLI_CHECK(data && scales && hi && lo && epi && groups && table, SLI_ERR_ARG,
              "sli_prefill_gemm_qkv_segs_mxfp4: null pointer");
    return pf_gemm_qkv_segs_entry(data, SLI_DT_MXFP4, scales, hi, lo, N, K, M, groups, B, epi, table, tiling, stream);
}

int sli_prefill_attn_segs(const float* q, const void* kc, const void* vc, int kv_dtype, void* ohi, void* olo, int32_t M,
                          const sli_pf_group* groups, int32_t B, int32_t hq, int32_t hkv, int32_t hd, int32_t T,
                          void* table, sli_stream_t stream) {
    SLI_CHECK(q && kc && vc && ohi && olo && groups && table, SLI_ERR_ARG, "sli_prefill_attn_segs: null pointer");
    SLI_CHECK(kv_dtype == SLI_DT_F16 || kv_dtype == SLI_DT_F8E4M3, SLI_ERR_ARG,
              "sli_prefill_attn_segs: an fp16 or FP8 cache (fp32 has no table form)");
    SLI_CHECK(pf_chunk_size(M), SLI_ERR_ARG, "sli_prefill_attn_segs: M must be 32, 64, 128 or 256");
    SLI_CHECK(hd == 64 || hd == 128, SLI_ERR_ARG, "sli_prefill_attn_segs: head_dim must be 64 or 128");
    SLI_CHECK(hq >= 1 && hkv >= 1 && hq % hkv == 0 && hq <= 65535, SLI_ERR_ARG,
              "sli_prefill_attn_segs: hq must be a multiple of hkv");
    SLI_CHECK(al16(q) && al16(kc) && al16(vc) && al16(ohi) && al16(olo), SLI_ERR_ARG,
              "sli_prefill_attn_segs: 16-byte alignment");
    hipStream_t s = as_stream(stream);
    if (int rc = pf_set_segs(table, groups, M, B, T, s)) return rc;
    return pf_attn_run(q, kc, vc, kv_dtype, ohi, olo, M, hq, hkv, hd, T, table, s);
}

// ---- scoring (score.h): the plain row map; sli_model_score_seqs launches the group-table one
int sli_score_rows(const float* logits, int32_t M, int32_t V, int32_t ld, const int32_t* targets, float* logprob,
                   int32_t* top, float* top_logprob, sli_stream_t stream) {
    SLI_CHECK(logits && targets && logprob, SLI_ERR_ARG, "sli_score_rows: null pointer");
    SLI_CHECK(M >= 1 && V >= 1, SLI_ERR_ARG, "sli_score_rows: M and V must be positive");
    SLI_CHECK(ld >= V && ld % 4 == 0, SLI_ERR_ARG, "sli_score_rows: ld must be >= V and a multiple of 4");
    SLI_CHECK(al16(logits), SLI_ERR_ARG, "sli_score_rows: logits must be 16-byte aligned");
    SLI_HIP(launch_score_rows(logits, M, V, ld, ScPlain{targets}, logprob, top, top_logprob, as_stream(stream)));
    return SLI_OK;
}

}  // extern "C"
