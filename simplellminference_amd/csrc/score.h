// score.h — per-token log-probabilities of a chunk of logits rows (the rule: include/sli.h at sli_score_rows). The
// reference has no scoring (model.cpp:157-183 keeps the argmax alone); this is the engine's own addition, the reading
// end of the GEMM prefill's LM head (sli_model_score_seqs).
//
// score_rows_kernel: one 1024-thread workgroup per row (16 waves on the row's CU, four 16-byte loads in flight per
// lane: with 256 threads the launch took 2.8 times a plain read of the chunk, too few bytes in flight). ONE pass over
// the row with 16-byte loads (the row base and ld
// are multiples of 4 floats, so a float4 never straddles the row's end by more than its own padding; the elements at
// V .. are masked to -inf / key 0, not branched around). A thread keeps an online (m, s) pair (s = sum exp(l - m)) and
// the largest common.h argmax_key of what it read; the waves reduce through the DPP helpers (the key through
// wave_max_u64), and the sixteen wave results meet in LDS, where thread 0 merges them in wave order. Every sum has one
// fixed order that depends on V alone: a row's result is bitwise the same from run to run and in any launch. No
// atomics, no workspace. The target logit and the top logit are one extra load each by thread 0.
// The launch is bound by one read of the chunk, M V 4 bytes (131 MB at 256 rows of a 128 256 vocabulary).
//
// One body, two row maps:
//   ScPlain  row m has target targets[m] and writes slot m;
//   ScSegs   row m = 16 g + r is position p0[g] + r of sequence seq[g] (the group table of sli_model_prefill_seqs): its
//            target is the NEXT prompt token, prompt[seq pld + p0 + r + 1], its slot (seq, p0 + r + 1) of
//            position-indexed buffers [B][pld]; a row with r >= nv[g] leaves at once (uniform, ahead of any barrier).
#pragma once
#include "common.h"
#include "prefill.h"

namespace sli {

constexpr int kScoreThreads = 1024;
constexpr int kScoreUnroll = 4;  // 16-byte loads in flight per thread

struct ScPlain {
    const int32_t* targets;
    __device__ __forceinline__ bool live(int) const { return true; }
    __device__ __forceinline__ size_t slot(int m) const { return (size_t)m; }
    __device__ __forceinline__ int target(int m) const { return targets[m]; }
};
struct ScSegs {
    const PfSegs* segs;
    const int32_t* prompt;  // [B][pld]
    int pld;
    __device__ __forceinline__ bool live(int m) const { return (m & 15) < segs->nv[m >> 4]; }
    __device__ __forceinline__ size_t slot(int m) const {
        const int g = m >> 4;
        return (size_t)segs->seq[g] * pld + segs->p0[g] + (m & 15) + 1;
    }
    __device__ __forceinline__ int target(int m) const { return prompt[slot(m)]; }
};

// exp(a - b) where b is a running maximum: a maximum of -inf (nothing but -inf so far) stands in as 0, so -inf terms
// give 0 and not exp(-inf + inf); a NaN stays a NaN
__device__ __forceinline__ float score_ref_max(float m) { return m == -INFINITY ? 0.0f : m; }

template <class RM>
__global__ void __launch_bounds__(kScoreThreads)
    score_rows_kernel(const float* __restrict__ logits, int V, int ld, RM rm, float* __restrict__ logprob,
                      int32_t* __restrict__ top, float* __restrict__ top_logprob) {
    const int m = blockIdx.x;
    if (!rm.live(m)) return;
    const float* row = logits + (size_t)m * ld;
    const int n4 = (V + 3) >> 2;  // float4 of the row; the last one may reach into the padding (ld % 4 == 0, ld >= V)
    float mx = -INFINITY, s = 0.0f;
    unsigned long long best = 0;
    for (int j0 = threadIdx.x; j0 < n4; j0 += kScoreThreads * kScoreUnroll) {
        float4 v4[kScoreUnroll];
#pragma unroll
        for (int u = 0; u < kScoreUnroll; ++u)  // past the row: the row's last float4 again, masked below
            v4[u] = reinterpret_cast<const float4*>(row)[min(j0 + u * kScoreThreads, n4 - 1)];
#pragma unroll
        for (int u = 0; u < kScoreUnroll; ++u) {
            const int j = j0 + u * kScoreThreads;
            const int i = 4 * j;
            const int nvalid = j < n4 ? V - i : 0;  // >= 4 but in the row's last float4
            float v[4] = {v4[u].x, v4[u].y, v4[u].z, v4[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = e < nvalid;
                v[e] = in ? v[e] : -INFINITY;
                const unsigned long long k = in ? argmax_key(v[e], (unsigned)(i + e)) : 0ull;
                best = k > best ? k : best;
            }
            const float mn = fmaxf(mx, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
            const float mm = score_ref_max(mn);
            s = s * expf(mx - mm) + ((expf(v[0] - mm) + expf(v[1] - mm)) + (expf(v[2] - mm) + expf(v[3] - mm)));
            mx = mn;
        }
    }
    // the wave: its maximum, the lanes' sums rescaled to it and added by the DPP tree
    const float wm = wave_max(mx);
    const float ws = wave_sum(s * expf(mx - score_ref_max(wm)));
    best = wave_max_u64(best);
    constexpr int NW = kScoreThreads / kWave;
    __shared__ float sh_m[NW], sh_s[NW];
    __shared__ unsigned long long sh_k[NW];
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sh_m[threadIdx.x / kWave] = wm;
        sh_s[threadIdx.x / kWave] = ws;
        sh_k[threadIdx.x / kWave] = best;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float M = sh_m[0];
    unsigned long long k = sh_k[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        M = fmaxf(M, sh_m[w]);
        k = sh_k[w] > k ? sh_k[w] : k;
    }
    const float Mm = score_ref_max(M);
    float S = sh_s[0] * expf(sh_m[0] - Mm);
#pragma unroll
    for (int w = 1; w < NW; ++w) S += sh_s[w] * expf(sh_m[w] - Mm);  // wave order
    const float lse = M + logf(S);
    // the target is never turned into an address unless it names a logit of the row
    const int t = rm.target(m);
    const bool t_ok = (unsigned)t < (unsigned)V;
    const float lt = row[t_ok ? t : 0];
    const size_t o = rm.slot(m);
    logprob[o] = t_ok ? lt - lse : __uint_as_float(0x7FC00000u);
    const unsigned ti = min(argmax_key_index(k), (unsigned)(V - 1));  // (index 0 always carries a key above 0)
    if (top) top[o] = (int32_t)ti;
    if (top_logprob) top_logprob[o] = row[ti] - lse;
}

template <class RM>
hipError_t launch_score_rows(const float* logits, int M, int V, int ld, const RM& rm, float* logprob, int32_t* top,
                             float* top_logprob, hipStream_t s) {
    hipLaunchKernelGGL((score_rows_kernel<RM>), dim3(M), dim3(kScoreThreads), 0, s, logits, V, ld, rm, logprob, top,
                       top_logprob);
    return hipGetLastError();
}

}  // namespace sli
