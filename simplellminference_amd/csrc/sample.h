// sample.h — seeded temperature / top-k / top-p sampling of one token per logits row (the rule: include/sli.h at
// sli_sample). The reference decodes greedily only (model.cpp:157-183); this is the engine's own addition, and it ends
// in an argmax like the rest of the step's tail: the Gumbel-max draw over the candidate set.
//
// One 1024-thread workgroup per row. A row does not fit the LDS (128 256 floats = 513 KB), so every pass re-reads it
// with 16-byte loads; right after the LM head it is L2-resident. The passes, each skipped where its stage is off:
//   1      the row maximum (as the orderable image of common.h argmax_key: -0 = +0, NaN at the bottom). No finite
//          maximum: one more pass computes sli_argmax's answer and the row is done.
//   2..4   top-k: radix select of the k-th largest image, digits of 11, 11 and 10 bits, integer LDS histograms;
//   5..7   top-p: the same descent over per-bin probability mass. A mass is exp((l - m) / T) * 2^40 truncated to an
//          integer and the bins are 64-bit integer LDS atomics, so every sum is exact and independent of the order in
//          which the lanes arrive: the threshold, hence the token, is bitwise reproducible (float atomics are not).
//          Truncation loses below 2^-40 per element, under 1.2e-7 of the total at 128 256 elements;
//   8      the draw: the largest key l / T - log(-log(u)) over the candidates, first index among equals.
// The only scratch is LDS (16.3 KB static); a row needs no workspace.
// Included by ops.hip alone (the kernel is no template); the engine launches through ops_internal.h.
#pragma once
#include "../../include/sli_synth.h"
#include "common.h"

namespace sli {

constexpr int kSampleThreads = 1024;
constexpr int kSampleBins = 2048;                  // 11-bit digits
constexpr unsigned kSampleOrdFiniteMin = 0x00800000u;  // image of -FLT_MAX: every finite value is at or above it
constexpr unsigned kSampleOrdPosInf = 0xFF800000u;     // image of +inf

// orderable image of a logit: larger float <=> larger image; -0 is +0; NaN is 0 (below -inf's 0x007FFFFF)
__device__ __forceinline__ unsigned sample_ord(float v) {
    if (v != v) return 0u;
    unsigned u = __float_as_uint(v);
    u = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sample_ord_value(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// f(value, index) for every element of the row, each exactly once: the 16-byte aligned middle as float4 loads, the
// up to three elements before and after it singly (a row may start at any float: row_stride is free)
template <class F>
__device__ __forceinline__ void sample_row_each(const float* __restrict__ row, int V, F f) {
    const int t = threadIdx.x;
    int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    head = head < V ? head : V;
    if (t < head) f(row[t], t);
    const int nv = (V - head) >> 2;
    const float4* p = reinterpret_cast<const float4*>(row + head);
    for (int j = t; j < nv; j += kSampleThreads) {
        const float4 v = p[j];
        const int i = head + 4 * j;
        f(v.x, i);
        f(v.y, i + 1);
        f(v.z, i + 2);
        f(v.w, i + 3);
    }
    const int tail = head + 4 * nv + t;
    if (t < 4 && tail < V) f(row[tail], tail);
}

struct SampleShared {
    unsigned long long hist[kSampleBins];  // counts (top-k) or masses (top-p) of the current digit
    unsigned long long wave[kSampleThreads / kWave];
    unsigned long long bc[2];
};

__device__ __forceinline__ unsigned long long sample_block_max(unsigned long long v, SampleShared& sh) {
    v = wave_max_u64(v);
    __syncthreads();  // sh.wave / sh.bc may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) sh.wave[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = 0;
        for (int w = 0; w < kSampleThreads / kWave; ++w) b = sh.wave[w] > b ? sh.wave[w] : b;
        sh.bc[0] = b;
    }
    __syncthreads();
    return sh.bc[0];
}

// The digit of the descent: the highest bin b whose suffix sum hist[b] + hist[b + 1] + ... reaches `target`
// (1 <= target <= the sum of all bins). Returns b; `above` = the sum of the bins above b, `total` = of all bins.
// Thread t owns bins 2047 - 2t and 2046 - 2t, so an inclusive scan over the threads is a suffix sum from the top.
__device__ __forceinline__ int sample_find_bin(SampleShared& sh, unsigned long long target, unsigned long long& above,
                                               unsigned long long& total) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    __syncthreads();  // the histogram is complete
    const unsigned long long h0 = sh.hist[kSampleBins - 1 - 2 * t], h1 = sh.hist[kSampleBins - 2 - 2 * t];
    unsigned long long inc = h0 + h1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += up;
    }
    if (lane == 63) sh.wave[w] = inc;
    __syncthreads();
    unsigned long long base = 0, all = 0;
    for (int i = 0; i < kSampleThreads / kWave; ++i) {
        const unsigned long long s = sh.wave[i];
        if (i < w) base += s;
        all += s;
    }
    inc += base;
    const unsigned long long exc = inc - (h0 + h1);
    if (exc < target && target <= inc) {  // exactly one thread: the suffix sums are non-decreasing
        const bool first = exc + h0 >= target;
        sh.bc[0] = (unsigned long long)(first ? kSampleBins - 1 - 2 * t : kSampleBins - 2 - 2 * t);
        sh.bc[1] = first ? exc : exc + h0;
    }
    __syncthreads();
    above = sh.bc[1];
    total = all;
    return (int)sh.bc[0];
}

__device__ __forceinline__ void sample_clear_hist(SampleShared& sh) {
    __syncthreads();  // the previous digit's readers are done
    sh.hist[threadIdx.x] = 0;
    sh.hist[threadIdx.x + kSampleThreads] = 0;
    __syncthreads();
}

// the three digits of an image, most significant first: bits 31..21, 20..10, 9..0
__device__ __forceinline__ int sample_digit(unsigned ord, int level) {
    return level == 0 ? (int)(ord >> 21) : level == 1 ? (int)((ord >> 10) & 2047u) : (int)(ord & 1023u);
}
// the bits above a level's digit (the prefix an element must share with the threshold found so far)
__device__ __forceinline__ unsigned sample_prefix_mask(int level) {
    return level == 0 ? 0u : level == 1 ? 0xFFE00000u : 0xFFFFFC00u;
}
__device__ __forceinline__ int sample_digit_shift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }

// The rule for one row, shared by sample_kernel and gen_sample.h's per-row kernel: each(f) calls f(value, index) for
// every element of the row exactly once, in any pass (the row itself, or its penalised values). Returns the token in
// every thread. GEN adds what sli_sample_gen's rule adds: temperature 0 (the argmax of the row is the answer) and
// min-p in the draw pass (min_p_on, c = log(min_p)); without GEN both are compiled out and the arguments unused.
template <bool GEN, class Each>
__device__ __forceinline__ int32_t sample_row(Each each, int V, float T, int top_k, float top_p, uint32_t seed,
                                              bool min_p_on, float c, int seq, const int32_t* __restrict__ posp,
                                              SampleShared& sh) {
    // ---- pass 1: the maximum
    unsigned mo = 0;
    bool greedy = false;
    if constexpr (GEN) greedy = T == 0.0f;
    if (!greedy) {
        each([&](float v, int) {
            const unsigned o = sample_ord(v);
            mo = o > mo ? o : mo;
        });
        mo = (unsigned)sample_block_max(mo, sh);
    }
    if (greedy || mo < kSampleOrdFiniteMin || mo >= kSampleOrdPosInf) {  // no finite maximum: sli_argmax's answer
        unsigned long long best = 0;
        each([&](float v, int i) {
            const unsigned long long k = argmax_key(v, (unsigned)i);
            best = k > best ? k : best;
        });
        best = sample_block_max(best, sh);
        return (int32_t)argmax_key_index(best);
    }
    const float m = sample_ord_value(mo);
    unsigned lo = kSampleOrdFiniteMin;  // candidates: image >= lo

    // ---- top-k: the image of the k-th largest element
    if (top_k > 0 && top_k < V) {
        unsigned thr = 0;
        unsigned long long need = (unsigned long long)top_k;
        for (int level = 0; level < 3; ++level) {
            sample_clear_hist(sh);
            const unsigned mask = sample_prefix_mask(level);
            each([&](float v, int) {
                const unsigned o = sample_ord(v);
                if ((o & mask) == thr) atomicAdd(&sh.hist[sample_digit(o, level)], 1ull);
            });
            unsigned long long above, total;
            const int b = sample_find_bin(sh, need, above, total);
            need -= above;
            thr |= (unsigned)b << sample_digit_shift(level);
        }
        lo = thr > lo ? thr : lo;
    }

    // ---- top-p over the top-k set: the largest image whose upper mass reaches top_p of the whole
    if (top_p < 1.0f) {
        unsigned thr = 0;
        unsigned long long need = 0;
        for (int level = 0; level < 3; ++level) {
            sample_clear_hist(sh);
            const unsigned mask = sample_prefix_mask(level);
            each([&](float v, int) {
                const unsigned o = sample_ord(v);
                if (o >= lo && (o & mask) == thr) {
                    const float w = expf(__fdiv_rn(__fsub_rn(v, m), T));  // in (0, 1]; the maximum gives 1
                    atomicAdd(&sh.hist[sample_digit(o, level)], (unsigned long long)(w * 1099511627776.0f));
                }
            });
            unsigned long long above, total;
            if (level == 0) {
                // the whole mass Z is only known after this scan: find the bin against Z itself first (its `total`),
                // then against the target ceil(top_p * Z), at least 1 and at most Z (Z >= 2^40: the maximum's mass)
                (void)sample_find_bin(sh, 1ull, above, total);
                const double want = ceil((double)top_p * (double)total);
                need = (unsigned long long)want;
                need = need < 1ull ? 1ull : need > total ? total : need;
            }
            const int b = sample_find_bin(sh, need, above, total);
            need -= above;
            thr |= (unsigned)b << sample_digit_shift(level);
        }
        lo = thr > lo ? thr : lo;
    }

    // ---- the draw: Gumbel-max over the candidates (GEN: those that pass min-p; the maximum always does)
    const int32_t p = *posp;
    const uint32_t stream = ((uint32_t)SLI_SAMPLE_STREAM << 16) | ((uint32_t)seq & 0xFFFFu);
    const uint64_t hi = (uint64_t)(uint32_t)p << 32;
    unsigned long long best = 0;
    each([&](float v, int i) {
        if (sample_ord(v) < lo) return;
        if constexpr (GEN) {
            if (min_p_on && !(__fdiv_rn(__fsub_rn(v, m), T) >= c)) return;
        }
        const uint32_t h = sli_rng_u32(seed, stream, hi | (uint32_t)i);
        const float u = (float)(2u * (h >> 9) + 1u) * 5.9604644775390625e-08f;  // exact: an odd 24-bit integer * 2^-24
        const float key = __fsub_rn(__fdiv_rn(v, T), logf(-logf(u)));
        const unsigned long long k = argmax_key(key, (unsigned)i);
        best = k > best ? k : best;
    });
    best = sample_block_max(best, sh);
    return (int32_t)argmax_key_index(best);
}

// Row r of the launch: sequence seq0 + r at position pos[r * pos_stride]. pd != null: the parameters are read from
// device memory (the engine's graph), else pv holds them.
__global__ void __launch_bounds__(kSampleThreads)
    sample_kernel(const float* __restrict__ logits, long long row_stride, int V, sli_sampling pv,
                  const sli_sampling* __restrict__ pd, int seq0, const int32_t* __restrict__ pos, int pos_stride,
                  int32_t* __restrict__ out) {
    __shared__ SampleShared sh;
    const int r = blockIdx.x;
    const float* row = logits + (long long)r * row_stride;
    const sli_sampling prm = pd ? *pd : pv;
    const int32_t tok = sample_row<false>([&](auto f) { sample_row_each(row, V, f); }, V, prm.temperature, prm.top_k,
                                          prm.top_p, prm.seed, false, 0.0f, seq0 + r, pos + (long long)r * pos_stride, sh);
    if (threadIdx.x == 0) out[r] = tok;
}

// the argument ranges of sli.h, host only: null, or what is wrong (a NaN fails every comparison)
const char* sample_params_error(const sli_sampling& p) {
    if (!(p.temperature >= 1e-2f && p.temperature <= 1e2f)) return "temperature outside [1e-2, 1e2]";
    if (!(p.top_p > 0.0f && p.top_p <= 1.0f)) return "top_p outside (0, 1]";
    if (p.top_k < 0) return "top_k < 0";
    return nullptr;
}

hipError_t launch_sample(const float* logits, long long row_stride, int rows, int V, const sli_sampling& pv,
                                const sli_sampling* pd, int seq0, const int32_t* pos, int pos_stride, int32_t* out,
                                hipStream_t s) {
    hipLaunchKernelGGL(sample_kernel, dim3(rows), dim3(kSampleThreads), 0, s, logits, row_stride, V, pv, pd, seq0, pos,
                       pos_stride, out);
    return hipGetLastError();
}

}  // namespace sli
