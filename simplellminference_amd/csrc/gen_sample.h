// gen_sample.h — the per-row sampler (the rule: include/sli.h at sli_sample_gen): every row of a launch has its own
// parameter block, and its logits may be penalised by the row's token history before sample.h's rule and min-p run
// on them. The rule's passes are sample.h's sample_row, the one body that sample_kernel instantiates over the plain row
// and this kernel over the penalised one; what this kernel adds:
//   * the penalised value of an element, available to every pass without a copy of the row. The workgroup first
//     builds, in dynamic LDS with integer atomics, a V-bit presence bitmap and an open-addressed (token, count) table
//     of the history window [penalty_from, pos]. A pass reads the four bitmap bits of a float4 and probes the table
//     only for an element whose bit is set; an element that is not in the window keeps its logit bit for bit. The
//     counts are integers, so the penalised values do not depend on the order in which the lanes arrive.
//   * min-p as one more test in the draw pass (sample_row<true>).
//   * the early exits: a row with temperature 0 and no penalty leaves at once and writes -1 (the caller's argmax key
//     names its token); temperature 0 with a penalty is one argmax pass over the penalised row.
// Capacity: a vocabulary of at most kGenMaxVocab (a 32 KB bitmap) and history rows of at most kGenMaxHist elements
// (8192 table slots, 64 KB); with SampleShared that is 114 836 B of the 160 KB a gfx950 workgroup may declare. A launch
// without a penalised row declares no dynamic LDS. Included by ops.hip alone; the engine launches through
// ops_internal.h.
#pragma once
#include "sample.h"

namespace sli {

constexpr int kGenMaxVocab = 262144;
constexpr int kGenMaxHist = 4097;  // a model of max_len 4096 keeps rows of max_len + 1
constexpr int kGenRowsPerLaunch = 8;  // parameter blocks passed by value per launch (sli_sample_gen)

// the table's size for history rows of n elements: the power of two at or above 1.5 n (a load of at most 2/3), 64 at
// the least
inline int gen_slots_log2(long long n) {
    int lg = 6;
    while ((1ll << lg) < n + n / 2) ++lg;
    return lg;
}
// one spare word: the four bits of a float4 may straddle two
__host__ __device__ inline int gen_bitmap_words(int V) { return (V + 31) / 32 + 1; }
inline size_t gen_lds_bytes(int V, long long hist_len) {
    return sizeof(unsigned) * ((size_t)gen_bitmap_words(V) + 2 * ((size_t)1 << gen_slots_log2(hist_len)));
}

struct GenRows {
    GenRow r[kGenRowsPerLaunch];
};

// the penalty of one row: the bitmap (null: the row is not penalised), the table (key = token + 1, 0 = empty) and the
// three coefficients
struct GenPen {
    const unsigned* bm;
    const unsigned* keys;
    const unsigned* cnt;
    unsigned mask;
    int shift;
    float rp, pp, fp;

    __device__ __forceinline__ static unsigned slot(unsigned key, int shift) { return (key * 2654435761u) >> shift; }
    // element i is in the window: its count, then the rule's three roundings
    __device__ __forceinline__ float one(float v, int i) const {
        const unsigned k = (unsigned)i + 1u;
        unsigned s = slot(k, shift);
        for (unsigned n = 0; n <= mask && keys[s] != k; ++n) s = (s + 1u) & mask;
        const float a = v > 0.0f ? __fdiv_rn(v, rp) : __fmul_rn(v, rp);
        return __fsub_rn(__fsub_rn(a, pp), __fmul_rn(fp, (float)cnt[s]));
    }
    __device__ __forceinline__ float at(float v, int i) const {
        return (bm[i >> 5] >> (i & 31)) & 1u ? one(v, i) : v;
    }
    __device__ __forceinline__ unsigned bits4(int i) const {
        const int sh = i & 31;
        unsigned w = bm[i >> 5] >> sh;
        if (sh > 28) w |= bm[(i >> 5) + 1] << (32 - sh);
        return w & 15u;
    }
};

// sample_row_each over the penalised row
template <class F>
__device__ __forceinline__ void gen_row_each(const float* __restrict__ row, int V, const GenPen& pen, F f) {
    const int t = threadIdx.x;
    const bool on = pen.bm != nullptr;
    int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
    head = head < V ? head : V;
    if (t < head) f(on ? pen.at(row[t], t) : row[t], t);
    const int nv = (V - head) >> 2;
    const float4* p = reinterpret_cast<const float4*>(row + head);
    for (int j = t; j < nv; j += kSampleThreads) {
        float4 v = p[j];
        const int i = head + 4 * j;
        const unsigned bits = on ? pen.bits4(i) : 0u;
        if (bits) {
            if (bits & 1u) v.x = pen.one(v.x, i);
            if (bits & 2u) v.y = pen.one(v.y, i + 1);
            if (bits & 4u) v.z = pen.one(v.z, i + 2);
            if (bits & 8u) v.w = pen.one(v.w, i + 3);
        }
        f(v.x, i);
        f(v.y, i + 1);
        f(v.z, i + 2);
        f(v.w, i + 3);
    }
    const int tail = head + 4 * nv + t;
    if (t < 4 && tail < V) f(on ? pen.at(row[tail], tail) : row[tail], tail);
}

// Row r of the launch: sequence seq0 + r at position pos[r * pos_stride], with block pd[r] (device memory: the engine's
// graph) or pv.r[r]. Its history is hist + r * hist_len, hist_len elements; slots_log2 == 0: the launch has no table
// (no row is penalised).
__global__ void __launch_bounds__(kSampleThreads)
    sample_gen_kernel(const float* __restrict__ logits, long long row_stride, int V, const GenRow* __restrict__ pd,
                      int seq0, const int32_t* __restrict__ pos, int pos_stride, const int32_t* __restrict__ hist,
                      long long hist_len, int slots_log2, int32_t* __restrict__ out, GenRows pv) {
    __shared__ SampleShared sh;
    extern __shared__ unsigned gen_lds[];
    const int r = blockIdx.x, t = threadIdx.x;
    const float* row = logits + (long long)r * row_stride;
    const GenRow prm = pd ? pd[r] : pv.r[r];
    const float T = prm.temperature;
    const bool penalised = slots_log2 > 0 && (prm.repetition_penalty != 1.0f || prm.presence_penalty != 0.0f ||
                                              prm.frequency_penalty != 0.0f);
    if (T == 0.0f && !penalised) {  // plain greedy: nothing to do here
        if (t == 0) out[r] = -1;
        return;
    }
    const int32_t p = pos[(long long)r * pos_stride];

    // ---- the history window [penalty_from, pos] as a bitmap and a count table
    GenPen pen{};
    if (penalised) {
        const int bw = gen_bitmap_words(V), slots = 1 << slots_log2;
        unsigned* bm = gen_lds;
        unsigned* keys = bm + bw;
        unsigned* cnt = keys + slots;
        for (int i = t; i < bw + 2 * slots; i += kSampleThreads) gen_lds[i] = 0u;
        __syncthreads();
        const unsigned mask = (unsigned)slots - 1u;
        const int shift = 32 - slots_log2;
        const int32_t* h = hist + (long long)r * hist_len;
        const long long last = p < hist_len - 1 ? p : hist_len - 1;  // the row holds hist_len elements
        for (long long j = (long long)(prm.penalty_from > 0 ? prm.penalty_from : 0) + t; j <= last; j += kSampleThreads) {
            const int32_t tok = h[j];
            if ((unsigned)tok >= (unsigned)V) continue;  // not counted, and no address is formed from it
            atomicOr(&bm[tok >> 5], 1u << (tok & 31));
            const unsigned k = (unsigned)tok + 1u;
            unsigned s = GenPen::slot(k, shift);
            for (unsigned n = 0; n <= mask; ++n) {  // at most hist_len keys in 1.5 hist_len slots: a slot is found
                const unsigned prev = atomicCAS(&keys[s], 0u, k);
                if (prev == 0u || prev == k) {
                    atomicAdd(&cnt[s], 1u);
                    break;
                }
                s = (s + 1u) & mask;
            }
        }
        __syncthreads();
        pen = GenPen{bm, keys, cnt, mask, shift, prm.repetition_penalty, prm.presence_penalty, prm.frequency_penalty};
    }

    // ---- sample.h's rule over the penalised row, with temperature 0 and min-p
    const int32_t tok = sample_row<true>([&](auto f) { gen_row_each(row, V, pen, f); }, V, T, prm.top_k, prm.top_p,
                                         prm.seed, prm.min_p != 0.0f, prm.log_min_p, seq0 + r,
                                         pos + (long long)r * pos_stride, sh);
    if (t == 0) out[r] = tok;
}

// the argument ranges of sli.h (the op's level: stop and max_pos are not looked at), host only
const char* gen_params_error(const sli_gen_params& p) {
    if (!(p.temperature == 0.0f || (p.temperature >= 1e-2f && p.temperature <= 1e2f)))
        return "temperature neither 0 nor in [1e-2, 1e2]";
    if (!(p.top_p > 0.0f && p.top_p <= 1.0f)) return "top_p outside (0, 1]";
    if (p.top_k < 0) return "top_k < 0";
    if (!(p.min_p >= 0.0f && p.min_p < 1.0f)) return "min_p outside [0, 1)";
    if (!(p.repetition_penalty >= 0.1f && p.repetition_penalty <= 10.0f)) return "repetition_penalty outside [0.1, 10]";
    if (!(p.presence_penalty >= -100.0f && p.presence_penalty <= 100.0f)) return "presence_penalty outside [-100, 100]";
    if (!(p.frequency_penalty >= -100.0f && p.frequency_penalty <= 100.0f))
        return "frequency_penalty outside [-100, 100]";
    if (p.penalty_from < 0) return "penalty_from < 0";
    if (p.n_stop < 0 || p.n_stop > SLI_MAX_STOP) return "n_stop outside [0, 8]";
    if (p.max_pos < 0) return "max_pos < 0";
    return nullptr;
}

bool gen_penalised(const sli_gen_params& p) {
    return p.repetition_penalty != 1.0f || p.presence_penalty != 0.0f || p.frequency_penalty != 0.0f;
}

GenRow gen_row(const sli_gen_params& p) {
    GenRow g{};
    g.temperature = p.temperature;
    g.top_k = p.top_k;
    g.top_p = p.top_p;
    g.seed = p.seed;
    g.min_p = p.min_p;
    g.log_min_p = p.min_p > 0.0f ? (float)std::log((double)p.min_p) : 0.0f;
    g.repetition_penalty = p.repetition_penalty;
    g.presence_penalty = p.presence_penalty;
    g.frequency_penalty = p.frequency_penalty;
    g.penalty_from = p.penalty_from;
    return g;
}

// null, or why the table cannot take vocabulary V and history rows of hist_len elements
const char* gen_capacity_error(int V, long long hist_len) {
    if (V > kGenMaxVocab) return "a penalised row takes a vocabulary of at most 262144 (its presence bitmap)";
    if (hist_len > kGenMaxHist) return "a penalised row takes history rows of at most 4097 elements (its count table)";
    return nullptr;
}

// pd != null: `rows` blocks in device memory, one launch. Otherwise pv: `rows` host blocks, passed by value eight to a
// launch. table: whether any row may be penalised (the dynamic LDS of the bitmap and the table is declared).
hipError_t launch_sample_gen(const float* logits, long long row_stride, int rows, int V, const GenRow* pv,
                             const GenRow* pd, int seq0, const int32_t* pos, int pos_stride, const int32_t* hist,
                             long long hist_len, bool table, int32_t* out, hipStream_t s) {
    const size_t lds = table ? gen_lds_bytes(V, hist_len) : 0;
    if (lds) {  // per launch: the attribute belongs to the current device, and a process may hold models on several
        const hipError_t allow = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_gen_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)gen_lds_bytes(kGenMaxVocab, kGenMaxHist));
        if (allow != hipSuccess) return allow;
    }
    const int lg = table ? gen_slots_log2(hist_len) : 0;
    if (pd) {
        hipLaunchKernelGGL(sample_gen_kernel, dim3(rows), dim3(kSampleThreads), lds, s, logits, row_stride, V, pd, seq0,
                           pos, pos_stride, hist, hist_len, lg, out, GenRows{});
        return hipGetLastError();
    }
    for (int r0 = 0; r0 < rows; r0 += kGenRowsPerLaunch) {
        const int n = rows - r0 < kGenRowsPerLaunch ? rows - r0 : kGenRowsPerLaunch;
        GenRows g{};
        for (int i = 0; i < n; ++i) g.r[i] = pv[r0 + i];
        hipLaunchKernelGGL(sample_gen_kernel, dim3(n), dim3(kSampleThreads), lds, s, logits + (long long)r0 * row_stride,
                           row_stride, V, (const GenRow*)nullptr, seq0 + r0, pos + (long long)r0 * pos_stride,
                           pos_stride, hist ? hist + (long long)r0 * hist_len : nullptr, hist_len, lg, out + r0, g);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sli
