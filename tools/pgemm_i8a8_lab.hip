// pgemm_i8a8_lab — tiling sweep of the integer-MFMA prefill GEMM (csrc/pgemm_i8a8.h pgemm_i8a8_kernel) on the
// Llama-2-7B projection shapes at every chunk size, and the two quantisers at M = 256: device time per launch (HIP
// events, 20 launches, the weights rotated over four copies so they stream from HBM as in the engine). Random codes,
// the plain-store epilogue: timing only. The winners per (shape, M) fill pg_i8a8_pick.
// --layout: instead, the lane layout of v_mfma_i32_16x16x64_i8 read off the hardware with one-hot operands: which
// (lane group, byte) of B meets each (lane group, byte) of A, and where C[i][n] lands.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Xclang -target-feature -Xclang -packed-fp32-ops \
//         -I simplellminference_amd/csrc -I include tools/pgemm_i8a8_lab.hip -o tools/pgemm_i8a8_lab
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pgemm_i8a8.h"

using namespace sli;

#define CK(x)                                                                                 \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

__global__ void lab_fill(uint8_t* p, size_t n, unsigned seed) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        p[i] = (uint8_t)(((unsigned)(i * 2654435761u) ^ seed ^ (unsigned)(i >> 7)) % 255 + 1);  // any byte: the time does not depend on the codes
}
static uint8_t* lab_buf(size_t n, unsigned seed) {
    uint8_t* p;
    CK(hipMalloc(&p, n));
    hipLaunchKernelGGL(lab_fill, dim3(1024), dim3(256), 0, 0, p, n, seed);
    CK(hipGetLastError());
    return p;
}
template <class F>
static float lab_time(F&& launch, int iters = 20) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int i = 0; i < 4; ++i) launch(i);
    CK(hipEventRecord(a, 0));
    for (int i = 0; i < iters; ++i) launch(i);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms * 1e3f / iters;
}

struct Shape {
    const char* name;
    int N, K;
};
constexpr int kCopies = 4;
struct Bufs {
    uint8_t *W[kCopies], *A;
    float *As, *y;
};

template <class Cfg>
static void run(const Shape& sh, int M, const Bufs& b) {
    using Geo = PgI8A8Geo<Cfg>;
    if (M % Geo::BM) return;
    using K = PgEpiLogits;
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pgemm_i8a8_kernel<K, Cfg>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)Geo::LDS));
    const K e{b.y, nullptr, sh.N, sh.N};
    const float us = lab_time([&](int i) {
        const PgI8A8In in{(const int8_t*)b.W[i % kCopies], (const int8_t*)b.A, b.As, sh.N, sh.K, M};
        CK((launch_pgemm_i8a8<K, Cfg>(in, e, 0)));
    });
    printf("%-8s M %3d  BM %3d WR %d WP %d S %d AT %d  lds %6zu  %8.2f us  %7.1f TOP/s\n", sh.name, M, Geo::BM, Geo::WR,
           Geo::WP, Geo::S, Geo::AT, Geo::LDS, us, 2.0 * sh.N * sh.K * M / us * 1e-6);
}

// ---------------------------------------------------------------- --layout
// meet[ka][kb] (ka = 16 group + byte of A at row 0, kb the same of B at chunk row 0): C[0][0] of the one-hot pair;
// cpos[i][n]: the index 4 lane + register at which C[i][n] of all-ones rows i (A) and n (B) lands
__global__ void __launch_bounds__(64) lab_layout(int* meet, int* cpos) {
    const int lane = threadIdx.x, row = lane & 15, kg = lane >> 4;
    for (int ka = 0; ka < 64; ++ka)
        for (int kb = 0; kb < 64; ++kb) {
            pg_i8a8_i4 a{0, 0, 0, 0}, b{0, 0, 0, 0};
            if (row == 0 && kg == (ka >> 4)) a[(ka & 15) >> 2] = 1 << (8 * (ka & 3));
            if (row == 0 && kg == (kb >> 4)) b[(kb & 15) >> 2] = 1 << (8 * (kb & 3));
            const pg_i8a8_i4 c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, pg_i8a8_i4{0, 0, 0, 0}, 0, 0, 0);
            if (lane == 0) meet[ka * 64 + kb] = c[0];
        }
    for (int i = 0; i < 16; ++i)
        for (int n = 0; n < 16; ++n) {
            const int ones = 0x01010101;
            const pg_i8a8_i4 a = row == i ? pg_i8a8_i4{ones, ones, ones, ones} : pg_i8a8_i4{0, 0, 0, 0};
            const pg_i8a8_i4 b = row == n ? pg_i8a8_i4{ones, ones, ones, ones} : pg_i8a8_i4{0, 0, 0, 0};
            const pg_i8a8_i4 c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, pg_i8a8_i4{0, 0, 0, 0}, 0, 0, 0);
            for (int r = 0; r < 4; ++r)
                if (c[r] == 64) cpos[i * 16 + n] = 4 * lane + r;  // one lane and register holds the 64
        }
}

static int layout() {
    int *meet, *cpos;
    CK(hipMalloc(&meet, sizeof(int) * 64 * 64));
    CK(hipMalloc(&cpos, sizeof(int) * 256));
    CK(hipMemset(cpos, 0xff, sizeof(int) * 256));
    hipLaunchKernelGGL(lab_layout, dim3(1), dim3(64), 0, 0, meet, cpos);
    CK(hipGetLastError());
    std::vector<int> hm(64 * 64), hc(256);
    CK(hipMemcpy(hm.data(), meet, sizeof(int) * hm.size(), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hc.data(), cpos, sizeof(int) * hc.size(), hipMemcpyDeviceToHost));
    bool same = true, cstd = true;
    for (int ka = 0; ka < 64; ++ka) {
        int hits = 0, at = -1;
        for (int kb = 0; kb < 64; ++kb)
            if (hm[ka * 64 + kb]) ++hits, at = kb;
        if (hits != 1 || at != ka) same = false;
        if (hits != 1 || at != ka) printf("A (group %d, byte %2d) meets %d B slots, last (group %d, byte %2d)\n", ka >> 4, ka & 15, hits, at >> 4, at & 15);
    }
    for (int i = 0; i < 16; ++i)
        for (int n = 0; n < 16; ++n)
            if (hc[i * 16 + n] != 4 * (n + 16 * (i / 4)) + i % 4) {
                cstd = false;
                printf("C[%d][%d] at lane %d register %d\n", i, n, hc[i * 16 + n] / 4, hc[i * 16 + n] % 4);
            }
    printf("A (group g, byte j) meets B (group g, byte j) and no other slot, for all 64: %s\n", same ? "yes" : "NO");
    printf("C[i][n] in lane n + 16 (i / 4), register i %% 4 (the layout of v_mfma_f32_16x16x32_f16): %s\n", cstd ? "yes" : "NO");
    return same && cstd ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--layout")) return layout();
    const Shape shapes[] = {{"qkv", 12288, 4096}, {"gate_up", 22016, 4096}, {"wo", 4096, 4096}, {"down", 4096, 11008}};
    for (const Shape& sh : shapes) {
        Bufs b;
        for (int c = 0; c < kCopies; ++c) b.W[c] = lab_buf((size_t)sh.N * sh.K, 11 + c);
        b.A = lab_buf((size_t)256 * sh.K, 3);
        CK(hipMalloc(&b.As, sizeof(float) * 256));
        CK(hipMemset(b.As, 0x3c, sizeof(float) * 256));
        CK(hipMalloc(&b.y, sizeof(float) * 256 * sh.N));
        for (int M : kPfSizes) {
            run<Pg8Cfg<32, 2, 1, 4, 2>>(sh, M, b);
            run<Pg8Cfg<32, 4, 1, 4, 2>>(sh, M, b);
            run<Pg8Cfg<32, 2, 1, 4, 4>>(sh, M, b);
            run<Pg8Cfg<64, 2, 2, 4, 2>>(sh, M, b);
            run<Pg8Cfg<64, 2, 2, 3, 2>>(sh, M, b);
            run<Pg8Cfg<64, 4, 1, 4, 2>>(sh, M, b);
            run<Pg8Cfg<64, 2, 2, 4, 4>>(sh, M, b);
            run<Pg8Cfg<64, 2, 2, 3, 4>>(sh, M, b);
            run<Pg8Cfg<64, 4, 2, 4, 2>>(sh, M, b);
            run<Pg8Cfg<64, 2, 1, 4, 4>>(sh, M, b);
            run<Pg8Cfg<128, 2, 2, 3, 4>>(sh, M, b);
            run<Pg8Cfg<128, 2, 2, 4, 4>>(sh, M, b);
            run<Pg8Cfg<128, 4, 2, 3, 2>>(sh, M, b);
            run<Pg8Cfg<128, 2, 4, 3, 4>>(sh, M, b);
        }
        for (int c = 0; c < kCopies; ++c) CK(hipFree(b.W[c]));
        CK(hipFree(b.A));
        CK(hipFree(b.As));
        CK(hipFree(b.y));
    }
    // the quantisers at M = 256: the normed fp32 source at D = 4096, the pair source at D = 4096 and 11008
    float *x, *w, *sc;
    __half *hi, *lo;
    int8_t* codes;
    CK(hipMalloc(&x, sizeof(float) * 256 * 4096));
    CK(hipMalloc(&w, sizeof(float) * 4096));
    CK(hipMemset(x, 0x3c, sizeof(float) * 256 * 4096));
    CK(hipMemset(w, 0x3c, sizeof(float) * 4096));
    CK(hipMalloc(&hi, 2 * 256 * 11008));
    CK(hipMalloc(&lo, 2 * 256 * 11008));
    CK(hipMemset(hi, 0x3c, 2 * 256 * 11008));
    CK(hipMemset(lo, 0x1c, 2 * 256 * 11008));
    CK(hipMalloc(&codes, (size_t)256 * 11008));
    CK(hipMalloc(&sc, sizeof(float) * 256));
    printf("norm_quant  D  4096 M 256  %8.2f us\n", lab_time([&](int) {
               hipLaunchKernelGGL((pf_quant_i8_kernel<Mx8SrcF32, true>), dim3(256), dim3(256), 0, 0, Mx8SrcF32{x}, w, codes, sc,
                                  4096, 1e-5f);
           }));
    for (int D : {4096, 11008})
        printf("pair_quant  D %5d M 256  %8.2f us\n", D, lab_time([&](int) {
                   hipLaunchKernelGGL((pf_quant_i8_kernel<Mx8SrcPair, false>), dim3(256), dim3(256), 0, 0, Mx8SrcPair{hi, lo},
                                      (const float*)nullptr, codes, sc, D, 0.0f);
               }));
    CK(hipDeviceSynchronize());
    return 0;
}
