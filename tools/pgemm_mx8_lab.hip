// pgemm_mx8_lab — tiling sweep of the block-scaled MFMA prefill GEMM (csrc/pgemm_mx8.h pgemm_mx8_kernel) on the
// Llama-2-7B projection shapes at every chunk size, and the two quantisers at M = 256: device time per launch (HIP
// events, 20 launches, the weights rotated over four copies so they stream from HBM as in the engine). Random codes,
// the plain-store epilogue: timing only. The winners per (shape, M) fill pg8_pick.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Xclang -target-feature -Xclang -packed-fp32-ops \
//         -I simplellminference_amd/csrc -I include tools/pgemm_mx8_lab.hip -o tools/pgemm_mx8_lab
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pgemm_mx8.h"

using namespace sli;

#define CK(x)                                                                                 \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

__global__ void lab_fill(uint8_t* p, size_t n, unsigned seed, unsigned lo, unsigned span) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        p[i] = (uint8_t)(lo + ((unsigned)(i * 2654435761u) ^ seed ^ (unsigned)(i >> 7)) % span);
}
static uint8_t* lab_buf(size_t n, unsigned seed, unsigned lo, unsigned span) {
    uint8_t* p;
    CK(hipMalloc(&p, n));
    hipLaunchKernelGGL(lab_fill, dim3(1024), dim3(256), 0, 0, p, n, seed, lo, span);
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
    uint8_t *W[kCopies], *Ws[kCopies], *A, *As;
    float* y;
};

template <class Cfg>
static void run(const Shape& sh, int M, const Bufs& b) {
    using Geo = Pg8Geo<Cfg>;
    if (M % Geo::BM) return;
    using K = PgEpiLogits;
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pgemm_mx8_kernel<K, Cfg>),
                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)Geo::LDS));
    const K e{b.y, nullptr, sh.N, sh.N};
    const float us = lab_time([&](int i) {
        const Pg8In in{b.W[i % kCopies], b.Ws[i % kCopies], b.A, b.As, sh.N, sh.K, M};
        CK((launch_pgemm_mx8<K, Cfg>(in, e, 0)));
    });
    printf("%-8s M %3d  BM %3d WR %d WP %d S %d AT %d  lds %6zu  %8.2f us  %7.1f TFLOP/s\n", sh.name, M, Geo::BM, Geo::WR,
           Geo::WP, Geo::S, Geo::AT, Geo::LDS, us, 2.0 * sh.N * sh.K * M / us * 1e-6);
}

int main() {
    const Shape shapes[] = {{"qkv", 12288, 4096}, {"gate_up", 22016, 4096}, {"wo", 4096, 4096}, {"down", 4096, 11008}};
    for (const Shape& sh : shapes) {
        Bufs b;
        for (int c = 0; c < kCopies; ++c) {
            b.W[c] = lab_buf((size_t)sh.N * sh.K / 2, 11 + c, 0, 256);
            b.Ws[c] = lab_buf((size_t)sh.N * sh.K / 32, 5 + c, 118, 6);
        }
        b.A = lab_buf((size_t)256 * sh.K, 3, 0, 120);  // no NaN code
        b.As = lab_buf((size_t)256 * sh.K / 32, 9, 124, 6);
        CK(hipMalloc(&b.y, sizeof(float) * 256 * sh.N));
        for (int M : kPfSizes) {
            run<Pg8Cfg<32, 2, 1, 4, 2>>(sh, M, b);
            run<Pg8Cfg<32, 4, 1, 4, 2>>(sh, M, b);
            run<Pg8Cfg<32, 2, 1, 4, 4>>(sh, M, b);
            run<Pg8Cfg<64, 2, 2, 4, 2>>(sh, M, b);
            run<Pg8Cfg<64, 2, 2, 3, 2>>(sh, M, b);
            run<Pg8Cfg<64, 4, 1, 4, 2>>(sh, M, b);
            run<Pg8Cfg<64, 2, 2, 4, 4>>(sh, M, b);
            run<Pg8Cfg<64, 4, 2, 4, 2>>(sh, M, b);
            run<Pg8Cfg<64, 2, 1, 4, 4>>(sh, M, b);
            run<Pg8Cfg<128, 2, 2, 3, 4>>(sh, M, b);
            run<Pg8Cfg<128, 2, 2, 4, 4>>(sh, M, b);
            run<Pg8Cfg<128, 4, 2, 3, 2>>(sh, M, b);
            run<Pg8Cfg<128, 2, 4, 3, 4>>(sh, M, b);
            run<Pg8Cfg<128, 4, 2, 3, 4>>(sh, M, b);
        }
        for (int c = 0; c < kCopies; ++c) {
            CK(hipFree(b.W[c]));
            CK(hipFree(b.Ws[c]));
        }
        CK(hipFree(b.A));
        CK(hipFree(b.As));
        CK(hipFree(b.y));
    }
    // the quantisers at M = 256: the normed fp32 source at D = 4096, the pair source at D = 4096 and 11008
    float *x, *w;
    __half *hi, *lo;
    CK(hipMalloc(&x, sizeof(float) * 256 * 4096));
    CK(hipMalloc(&w, sizeof(float) * 4096));
    CK(hipMemset(x, 0x3c, sizeof(float) * 256 * 4096));
    CK(hipMemset(w, 0x3c, sizeof(float) * 4096));
    CK(hipMalloc(&hi, 2 * 256 * 11008));
    CK(hipMalloc(&lo, 2 * 256 * 11008));
    CK(hipMemset(hi, 0x3c, 2 * 256 * 11008));
    CK(hipMemset(lo, 0x1c, 2 * 256 * 11008));
    uint8_t *codes = lab_buf((size_t)256 * 11008, 1, 0, 1), *sc = lab_buf((size_t)256 * 11008 / 32, 1, 0, 1);
    printf("norm_quant  D  4096 M 256  %8.2f us\n", lab_time([&](int) {
               hipLaunchKernelGGL((pf_quant_mx8_kernel<Mx8SrcF32, true>), dim3(256), dim3(256), 0, 0, Mx8SrcF32{x}, w, codes,
                                  sc, 4096, 1e-5f);
           }));
    for (int D : {4096, 11008})
        printf("pair_quant  D %5d M 256  %8.2f us\n", D, lab_time([&](int) {
                   hipLaunchKernelGGL((pf_quant_mx8_kernel<Mx8SrcPair, false>), dim3(256), dim3(256), 0, 0,
                                      Mx8SrcPair{hi, lo}, (const float*)nullptr, codes, sc, D, 0.0f);
               }));
    CK(hipDeviceSynchronize());
    return 0;
}
