// pgemm_lab — tiling / ring-depth sweep of the prefill GEMM (csrc/prefill.h pgemm_kernel) on the Llama-2-7B
// projection shapes at a 256-row chunk: device time per launch (HIP events, 20 launches), issued MFMA
// TFLOP/s (hi + lo: 4 N K M), and a spot check of 64 outputs against a host fp64 sum. LAB_MX: the MXFP4 sweep.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I simplellminference_amd/csrc tools/pgemm_lab.hip -o tools/pgemm_lab
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prefill.h"

using namespace sli;

#define CK(x)                                                                          \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static uint32_t rng(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

struct Shape {
    const char* name;
    int N, K;
};

template <typename WT>
struct Bufs {
    std::vector<WT*> Wc;  // the timing loop rotates over copies (none MALL-resident: weights stream from HBM as in
                          // the engine, where a layer's weights are read once per chunk)
    std::vector<uint8_t*> Sc;  // mxfp4: the block scales of each copy
    __half *hi, *lo;
    float* y;
    std::vector<WT> hW;  // mxfp4: data [N][K/2], two codes per byte
    std::vector<uint8_t> hS;  // mxfp4: scale bytes 120 .. 126
    std::vector<__half> hhi, hlo;
};

static float h2f(__half h) { return __half2float(h); }

template <typename WT>
static const char* wt_name() {
    return is_mx<WT>::value ? "mxfp4" : sizeof(WT) == 1 ? "i8" : "f16";
}

// the weight W[row][k] as the kernel decodes it
template <typename WT>
static double w_host(const Bufs<WT>& b, int K, int row, int k) {
    if constexpr (is_mx<WT>::value) {
        static const double mag[8] = {0, .5, 1, 1.5, 2, 3, 4, 6};
        const uint8_t byte = b.hW[(size_t)row * (K / 2) + k / 2].b;
        const unsigned c = (k & 1) ? byte >> 4 : byte & 15;
        return ((c & 8) ? -mag[c & 7] : mag[c & 7]) * ldexp(1.0, (int)b.hS[(size_t)row * (K / 32) + k / 32] - 127);
    } else if constexpr (sizeof(WT) == 1) {
        return (double)b.hW[(size_t)row * K + k];
    } else {
        return (double)h2f(b.hW[(size_t)row * K + k]);
    }
}

template <typename WT>
static void make(Bufs<WT>& b, int N, int K, int M) {
    uint64_t s = (is_mx<WT>::value ? 999 : 12345) + N + K;
    b.hW.resize((size_t)N * wt_row_bytes<WT>(K) / sizeof(WT));
    for (auto& w : b.hW) {
        if constexpr (is_mx<WT>::value)
            w.b = (uint8_t)rng(s);
        else if constexpr (sizeof(WT) == 1)
            w = (int8_t)((int)(rng(s) % 255) - 127);
        else
            w = __float2half(((int)(rng(s) % 2001) - 1000) * 1e-3f * 0.05f);
    }
    if (is_mx<WT>::value) {
        b.hS.resize((size_t)N * K / 32);
        for (auto& w : b.hS) w = (uint8_t)(120 + rng(s) % 7);
    }
    b.hhi.resize((size_t)M * K);
    b.hlo.resize((size_t)M * K);
    for (size_t i = 0; i < b.hhi.size(); ++i) {
        const float v = ((int)(rng(s) % 200001) - 100000) * 1e-5f;
        b.hhi[i] = __float2half(v);
        b.hlo[i] = __float2half(v - __half2float(b.hhi[i]));
    }
    const int ncopy = getenv("LAB_HOT") ? 1 : 4;
    for (int c = 0; c < ncopy; ++c) {
        WT* w;
        CK(hipMalloc(&w, sizeof(WT) * b.hW.size()));
        CK(hipMemcpy(w, b.hW.data(), sizeof(WT) * b.hW.size(), hipMemcpyHostToDevice));
        b.Wc.push_back(w);
        uint8_t* sc = nullptr;
        if (!b.hS.empty()) {
            CK(hipMalloc(&sc, b.hS.size()));
            CK(hipMemcpy(sc, b.hS.data(), b.hS.size(), hipMemcpyHostToDevice));
        }
        b.Sc.push_back(sc);
    }
    CK(hipMalloc(&b.hi, 2 * b.hhi.size()));
    CK(hipMalloc(&b.lo, 2 * b.hlo.size()));
    CK(hipMalloc(&b.y, sizeof(float) * (size_t)M * N));
    CK(hipMemcpy(b.hi, b.hhi.data(), 2 * b.hhi.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(b.lo, b.hlo.data(), 2 * b.hlo.size(), hipMemcpyHostToDevice));
}

template <typename WT>
static void release(Bufs<WT>& b) {
    for (auto* p : b.Wc) CK(hipFree(p));
    for (auto* p : b.Sc) CK(hipFree(p));
    CK(hipFree(b.hi));
    CK(hipFree(b.lo));
    CK(hipFree(b.y));
}

template <class Cfg, typename WT>
static void run(const char* tag, Bufs<WT>& b, const Shape& sh, int M) {
    using Geo = PgGeo<Cfg, WT>;
    if (M % Geo::BM) return;
    CK((pgemm_allow_lds<PgEpiResid, Cfg, WT>()));
    PgIn<WT> in{b.Wc[0], b.hi, b.lo, sh.N, sh.K, M, b.Sc[0]};
    PgEpiResid e{b.y, nullptr, nullptr, sh.N, sh.N};
    CK(hipMemset(b.y, 0, sizeof(float) * (size_t)M * sh.N));
    CK((launch_pgemm<PgEpiResid, Cfg, WT>(in, e, 0)));
    CK(hipDeviceSynchronize());
    // spot check (y[m][row] = sum_k W[row][k] (hi + lo)[m][k])
    std::vector<float> y((size_t)M * sh.N);
    CK(hipMemcpy(y.data(), b.y, sizeof(float) * y.size(), hipMemcpyDeviceToHost));
    double maxrel = 0.0;
    uint64_t s = 777;
    for (int i = 0; i < 64; ++i) {
        const int m = rng(s) % M, row = rng(s) % sh.N;
        double ref = 0.0, mag = 0.0;
        for (int k = 0; k < sh.K; ++k) {
            const double w = w_host(b, sh.K, row, k);
            const double x = (double)h2f(b.hhi[(size_t)m * sh.K + k]) + (double)h2f(b.hlo[(size_t)m * sh.K + k]);
            ref += w * x;
            mag += fabs(w * x);
        }
        maxrel = fmax(maxrel, fabs(y[(size_t)m * sh.N + row] - ref) / (mag + 1e-30));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const int iters = 20;
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < iters; ++i) {
        PgIn<WT> ic = in;
        ic.W = b.Wc[i % b.Wc.size()];
        ic.Ws = b.Sc[i % b.Sc.size()];
        CK((launch_pgemm<PgEpiResid, Cfg, WT>(ic, e, 0)));
    }
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms = 0.0f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    const double us = 1000.0 * ms / iters;
    const double tf = 4.0 * sh.N * sh.K * (double)M / (us * 1e-6) / 1e12;
    const double wgbs = (double)sh.N * wt_row_bytes<WT>(sh.K) / (us * 1e-6) / 1e9;
    const int nrb = (sh.N + Geo::BN - 1) / Geo::BN;
    printf("%-5s %-6s %-22s grid %5d lds %6zu  %8.1f us  %6.1f TF issued  W %6.0f GB/s  relerr %.1e\n", sh.name,
           wt_name<WT>(), tag, nrb * (M / Geo::BM), Geo::LDS, us, tf, wgbs, maxrel);
    fflush(stdout);
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
}

#define RUN(BM, WR, S) run<PgCfg<BM, WR, S>, WT>("BM" #BM " WR" #WR " S" #S, b, sh, M)
#define RUNT(BM, WR, S, AT) run<PgCfg<BM, WR, S, AT>, WT>("BM" #BM " WR" #WR " S" #S " AT" #AT, b, sh, M)
#define RUNP(BM, WR, S, AT) run<PgCfg<BM, WR, S, AT, true>, WT>("BM" #BM " WR" #WR " S" #S " AT" #AT " pipe", b, sh, M)
#define RUNA(BM, WR, AT, SA) \
    run<PgCfg<BM, WR, 2, AT, true, SA>, WT>("BM" #BM " WR" #WR " AT" #AT " pipe SA" #SA, b, sh, M)

template <typename WT>
static void sweep(const Shape& sh, int M) {
    Bufs<WT> b;
    make(b, sh.N, sh.K, M);
    if (getenv("LAB_QUICK")) {  // the engine's tilings at M = 256 (prefill.h pg_pick)
        if constexpr (is_mx<WT>::value) {
            RUNT(128, 4, 2, 2);
            RUNT(64, 4, 3, 2);
            RUNT(32, 4, 4, 2);
        } else if constexpr (sizeof(WT) == 2) {
            RUNA(128, 4, 2, 4);
            RUNP(64, 4, 3, 2);
            RUNP(64, 2, 3, 2);
        } else if (getenv("LAB_I8")) {
            RUNP(128, 4, 2, 2);
            RUNP(64, 4, 2, 2);
            RUNP(64, 2, 2, 2);
        }
    } else if constexpr (is_mx<WT>::value) {
        RUNT(128, 4, 2, 2);
        RUNT(128, 2, 2, 2);
        RUNT(64, 4, 2, 2);
        RUNT(64, 4, 3, 2);
        RUNT(64, 2, 2, 2);
        RUNT(64, 2, 3, 2);
        RUNT(64, 2, 4, 2);
        RUNT(64, 2, 2, 4);
        RUNT(32, 2, 4, 2);
        RUNT(32, 4, 4, 2);
        RUNP(64, 4, 3, 2);  // the pipelined fragment reads compile for this format too (no table cell uses them yet)
    } else if constexpr (sizeof(WT) == 2) {
        RUN(128, 2, 2);
        RUN(128, 2, 3);
        RUN(128, 2, 4);
        RUN(64, 2, 3);
        RUN(64, 2, 4);
        RUN(64, 2, 6);
        RUN(64, 4, 3);
        RUN(64, 4, 4);
        RUN(128, 4, 2);
        RUN(128, 4, 3);
        RUN(256, 2, 2);
        RUN(256, 4, 2);
        RUN(32, 2, 4);
        RUN(32, 2, 8);
    } else {
        RUN(64, 2, 2);
        RUN(64, 2, 3);
        RUN(128, 2, 2);
        RUN(64, 4, 2);
        RUN(64, 4, 3);
        RUN(128, 4, 2);
        RUN(32, 2, 4);
    }
    release(b);
}

int main(int argc, char** argv) {
    const int M = argc > 1 ? atoi(argv[1]) : 256;
    const Shape shapes[] = {{"qkv", 12288, 4096}, {"gu", 22016, 4096}, {"wo", 4096, 4096}, {"down", 4096, 11008}};
    if (getenv("LAB_MX")) {  // the MXFP4 format alone
        for (const Shape& sh : shapes) sweep<mxfp4>(sh, M);
        return 0;
    }
    for (const Shape& sh : shapes) sweep<__half>(sh, M);
    for (const Shape& sh : shapes) sweep<int8_t>(sh, M);
    return 0;
}
