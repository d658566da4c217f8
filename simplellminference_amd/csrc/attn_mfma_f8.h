// attn_mfma_f8.h — the MFMA decode attention of attn_mfma.h for an FP8 E4M3 K/V cache (SLI_DT_F8E4M3, one byte per
// element, no scale). The only attention an FP8 cache runs. Carried over unchanged: the workgroup (4 waves = one
// (kv head, context split), wave w owns the split's 32-key tiles w, w + 4, ...; a per-wave tile ring fed by LDS-DMA,
// no workgroup barrier in the loop), the q path (fp32 by LDS-DMA, three fp16 terms), the online softmax, P as three
// fp16 terms, the in-LDS wave merge, the partial layout and am_merge. What differs:
//
//   * a cache row is HD bytes, so a 32-key K + V tile is 8 KiB (hd 128) or 4 KiB (hd 64): half the fp16 kernel's
//     bytes per tile, which is why the ring depth NBUF goes up to 4 (the same bytes in flight per CU as the fp16
//     kernel's 2);
//   * the K operand: a lane reads the 8 codes of its row at d = 32 db + 8 g .. +7 (ds_read_b64) and widens them to
//     the exact fp16 A fragment in registers (common.h f8x8_to_f16); the MFMA stays v_mfma_f32_16x16x32_f16, so q
//     and P keep their three fp16 terms and the arithmetic after the widening is the fp16 kernel's;
//   * the V operand: ONE ds_read_b64_tr_b8 per 16-d tile. Per group of 16 lanes it reads a block of 8 rows x 16
//     one-byte columns: lane 2 q + p of the group (q = 0..7, p = 0..1) supplies the address of row q, columns
//     8 p .. 8 p + 7, and lane i receives column i of the 8 rows, row q in its byte q. Lane group g reads rows
//     8 g .. 8 g + 7, so a lane of the Vᵀ A operand holds d = 16 t + i16 of keys 8 g .. 8 g + 7 of the tile;
//   * the key <-> A-row map of the S MFMAs is chosen so that the S accumulators a lane holds are exactly those keys:
//     A row m of S MFMA kt is key 8 (m >> 2) + 4 kt + (m & 3), so lane group g's accumulator r of MFMA kt is key
//     8 g + 4 kt + r, element 4 kt + r of its Pᵀ B operand;
//   * the chunk swizzles are re-derived for the new row length (below).
//
// The two recorded hazards of attn_mfma.h hold here as well: the asm DMAs and asm LDS reads are invisible to the
// compiler's wait counting, so the waits are counted vmcnt and no other vector-memory load is issued while pieces
// are in flight; and the transposed reads' destination registers are "+v" operands of the lgkmcnt wait.
#pragma once
#include "attn_mfma.h"

namespace sli {

template <int HD, int G>
struct AmGeo8 {
    static constexpr int ROWB = HD;                  // bytes per cache row
    static constexpr int IMG = kAmKeys * ROWB;       // one 32-key K (or V) image
    static constexpr int TILE = 2 * IMG;             // K + V
    static constexpr int PIECES = TILE / 1024;       // 1-KiB DMA pieces per tile
    static constexpr int CPR = ROWB / 16;            // 16-B chunks per row
    static constexpr int QB = ((G * HD * 4 + 1023) / 1024) * 1024;  // the q image (fp32), whole pieces
    static constexpr int QP = QB / 1024;
    static constexpr int ND = HD / 32, NT = HD / 16;  // 32-d blocks (S), 16-d tiles (O)
    static constexpr int MERGE = (NT * 64 * 4 + 128) * 4;  // the wave's (o, mx, l) image of the in-LDS merge
    template <int NBUF>
    static constexpr int wave_bytes() { return QB + NBUF * TILE; }
    static_assert(HD == 64 || HD == 128, "head_dim");
    static_assert(G >= 1 && G <= 16, "query heads per kv head: one MFMA column each");
    static_assert(QB + TILE >= MERGE, "the merge image fits the smallest wave image");
};
// Chunk swizzles (physical 16-B chunk = logical chunk ^ swizzle(row)). Banks are counted per 32-lane half over the
// 256-byte bank row, i.e. 16 slots of 16 bytes; a row starts at slot 8 (r & 1) for 128-byte rows and 4 (r & 3) for
// 64-byte rows.
//   K: a half-wave's ds_read_b64 touches one logical chunk of the 16 rows 8 a + 4 kt + b (a, b = 0..3), two lanes
//      per chunk. 128-byte rows: slot 8 (b & 1) + (c ^ swz), so swz takes 8 values over (a, b >> 1); 64-byte rows:
//      slot 4 b + (c ^ swz), so swz takes 4 values over a.
//   V: a half-wave's transposed read touches one logical chunk of 16 consecutive rows r. 128-byte rows: slot
//      8 (r & 1) + (c ^ swz), swz = (r >> 1) & 7; 64-byte rows: slot 4 (r & 3) + (c ^ swz), swz = (r >> 2) & 3.
__device__ __forceinline__ int am8_swz_k(int r, int rowb) {
    return rowb == 128 ? (((r >> 3) & 3) << 1) | ((r >> 1) & 1) : (r >> 3) & 3;
}
__device__ __forceinline__ int am8_swz_v(int r, int rowb) { return rowb == 128 ? (r >> 1) & 7 : (r >> 2) & 3; }

__device__ __forceinline__ uint2 am_tr8_read(unsigned lds_addr) {
    uint2 v;
    asm volatile("ds_read_b64_tr_b8 %0, %1" : "=v"(v) : "v"(lds_addr) : "memory");
    return v;
}
// at most n tiles (of P pieces) still in flight
template <int P>
__device__ __forceinline__ void am8_wait_tiles(int n) {
    if (n <= 0)
        am_wait_vm<0>();
    else if (n == 1)
        am_wait_vm<P>();
    else if (n == 2)
        am_wait_vm<2 * P>();
    else if (n == 3)
        am_wait_vm<3 * P>();
    else
        am_wait_vm<4 * P>();
}

// grid: n_kv_heads (every sequence's) * max_splits workgroups of 256 threads; a.ppwg = kAmWgKeys * tpw (the split
// length), NBUF <= min(tpw, 4) ring slots per wave. Row indices are clamped to pos (rows past the live context
// re-read row pos and are masked).
template <int HD, int G, int NBUF>
__global__ void __launch_bounds__(64 * kAmWaves) attn_mfma_f8_kernel(AttnArgs<f8e4m3> a) {
    using Geo = AmGeo8<HD, G>;
    constexpr int ND = Geo::ND, NT = Geo::NT, P = Geo::PIECES;
    constexpr int WB = Geo::template wave_bytes<NBUF>();
    static_assert(NBUF >= 1 && NBUF <= 4 && 4 * P + Geo::QP <= 63, "vmcnt is 6 bits");
    __shared__ __attribute__((aligned(1024))) char sm[kAmWaves * WB];
    __shared__ int last;
    if (a.stamps && threadIdx.x == 0) a.stamps[blockIdx.x * 4] = __builtin_amdgcn_s_memrealtime();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = lane >> 4, i16 = lane & 15;
    const int kvh = blockIdx.x / a.max_splits, wgs = blockIdx.x - kvh * a.max_splits;
    const int pos = attn_pos(a, kvh);
    const int ppwg = a.ppwg;
    const int s0 = wgs * ppwg;
    if (s0 > pos) return;  // the whole split past the live context (uniform)
    const int tpw = ppwg / kAmWgKeys;
    const int rel = pos - s0;
    // live tiles of this wave: j with s0 + (4 j + wave) * 32 <= pos
    const int nl = rel >= wave * kAmKeys ? min(tpw, (rel / kAmKeys - wave) / kAmWaves + 1) : 0;

    char* wimg = sm + wave * WB;
    const unsigned wbase = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)wimg;
    const unsigned qbase = wbase, tbase = wbase + Geo::QB;
    const int ch = a.cache_heads > 0 ? kvh % a.cache_heads : kvh / a.kv_group;
    const char* kc = reinterpret_cast<const char*>(a.k) + (long long)ch * a.head_stride;
    const char* vc = reinterpret_cast<const char*>(a.v) + (long long)ch * a.head_stride;

    // tile j of this wave into ring slot j % NBUF: K pieces 0 .. P/2-1, V pieces P/2 .. P-1; lane i of a piece:
    // row (piece rows) + i / CPR, physical chunk i % CPR <- logical chunk (i % CPR) ^ swizzle(row)
    auto issue = [&](int j) {
        const int t0 = s0 + (kAmWaves * j + wave) * kAmKeys;
        const unsigned base = tbase + (unsigned)((j % NBUF) * Geo::TILE);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const bool isv = p >= P / 2;
            const int jj = isv ? p - P / 2 : p;
            const int r = jj * (1024 / Geo::ROWB) + lane / Geo::CPR;
            const int c = (lane % Geo::CPR) ^ (isv ? am8_swz_v(r, Geo::ROWB) : am8_swz_k(r, Geo::ROWB));
            const char* src = (isv ? vc : kc) + (long long)min(t0 + r, pos) * a.pos_stride + c * 16;
            am_dma<true>(src, base + (isv ? Geo::IMG : 0) + (unsigned)(jj * 1024));
        }
    };
    // q of the kv head's G query heads (fp32, contiguous): QP pieces, clamped inside the vector
    {
        const float* qs = a.q + (size_t)kvh * G * HD;
#pragma unroll
        for (int p = 0; p < Geo::QP; ++p)
            am_dma<false>(qs + min(p * 256 + lane * 4, G * HD - 4), qbase + (unsigned)(p * 1024));
    }
#pragma unroll
    for (int j = 0; j < NBUF; ++j)
        if (j < nl) issue(j);
    am8_wait_tiles<P>(min(nl, NBUF));  // q landed (the tiles may still be in flight)
    // Qᵀ as the B operand: lane l = query column l & 15 (q head kvh * G + col for col < G, else zero), d = 32 db +
    // 8 g .. +7, fp32 -> hi + mid + lo
    u32x4 qh[ND], qm[ND], ql[ND];
#pragma unroll
    for (int db = 0; db < ND; ++db) {
        float f[8];
        if (i16 < G) {
            const float4* qp = reinterpret_cast<const float4*>(wimg + 4 * (i16 * HD + db * 32 + g * 8));
            const float4 v0 = qp[0], v1 = qp[1];
            f[0] = v0.x, f[1] = v0.y, f[2] = v0.z, f[3] = v0.w, f[4] = v1.x, f[5] = v1.y, f[6] = v1.z, f[7] = v1.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = 0.0f;
        }
        __half hh[8], hm[8], hl[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) am_split3(f[e], hh[e], hm[e], hl[e]);
        qh[db] = *reinterpret_cast<const u32x4*>(hh);
        qm[db] = *reinterpret_cast<const u32x4*>(hm);
        ql[db] = *reinterpret_cast<const u32x4*>(hl);
    }
    am_float4 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) o[t] = am_float4{0.0f, 0.0f, 0.0f, 0.0f};
    float mx = -INFINITY, l = 0.0f;
    if (a.stamps && threadIdx.x == 0) a.stamps[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memrealtime();

    // the K row this lane feeds to S MFMA kt as A row i16: key 8 (i16 >> 2) + 4 kt + (i16 & 3) of the tile
    const int krow0 = 8 * (i16 >> 2) + (i16 & 3);
    // the V address of this lane for the transposed read: row 8 g + (i16 >> 1), 8 bytes at column 8 (i16 & 1) of a
    // 16-d chunk
    const int vrow = 8 * g + (i16 >> 1);
    const int vsw = am8_swz_v(vrow, Geo::ROWB);
    for (int j = 0; j < nl; ++j) {
        // tile j landed (up to NBUF - 1 later tiles may still be in flight)
        am8_wait_tiles<P>(min(nl - 1 - j, NBUF - 1));
        const int t0 = s0 + (kAmWaves * j + wave) * kAmKeys;
        const char* kimg = wimg + Geo::QB + (j % NBUF) * Geo::TILE;
        const unsigned vbase = tbase + (unsigned)((j % NBUF) * Geo::TILE) + Geo::IMG;
        // Sᵀ[key][query]
        am_float4 sacc[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            sacc[kt] = am_float4{0.0f, 0.0f, 0.0f, 0.0f};
            const int r = krow0 + 4 * kt;
            const char* krow = kimg + r * Geo::ROWB + 8 * (g & 1);
            const int sw = am8_swz_k(r, Geo::ROWB);
#pragma unroll
            for (int db = 0; db < ND; ++db) {
                const u32x2 kb = *reinterpret_cast<const u32x2*>(krow + ((2 * db + (g >> 1)) ^ sw) * 16);
                const u32x4 kf = f8x8_to_f16(kb.x, kb.y);
                sacc[kt] = am_mfma(kf, qh[db], sacc[kt]);
                sacc[kt] = am_mfma(kf, qm[db], sacc[kt]);
                sacc[kt] = am_mfma(kf, ql[db], sacc[kt]);
            }
        }
        // Vᵀ 16-d tile t (issued before the softmax so the LDS reads overlap it)
        const unsigned va = vbase + vrow * Geo::ROWB + 8 * (i16 & 1);
        uint2 x[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) x[t] = am_tr8_read(va + ((t ^ vsw) * 16));
        // lane holds keys t0 + 8 g + 4 kt + r of its query column (mha_kernel.cpp:51-60: s = (q . k) * scale)
        float sv[8];
        float cmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = t0 + 8 * g + 4 * kt + r;
                const float v = key <= pos ? sacc[kt][r] * a.scale : -INFINITY;
                sv[kt * 4 + r] = v;
                cmax = fmaxf(cmax, v);
            }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
        const float mn = fmaxf(mx, cmax);  // finite: a live tile holds key t0 <= pos
        const float corr = expf(mx - mn);  // 0 on the first tile (mx = -inf)
        float pv[8], psum = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            pv[e] = expf(sv[e] - mn);  // 0 for masked keys
            psum += pv[e];
        }
        psum += __shfl_xor(psum, 16);
        psum += __shfl_xor(psum, 32);
        l = l * corr + psum;
        mx = mn;
        __half ph[8], pm[8], pl[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) am_split3(pv[e], ph[e], pm[e], pl[e]);
        const u32x4 pfh = *reinterpret_cast<const u32x4*>(ph);
        const u32x4 pfm = *reinterpret_cast<const u32x4*>(pm);
        const u32x4 pfl = *reinterpret_cast<const u32x4*>(pl);
        // the transposed reads landed; their registers are named in the wait, so the compiler neither reads nor
        // copies them above it (attn_mfma.h, DESIGN.md §9 fault record)
        if constexpr (NT == 8)
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
                         :
                         : "memory");
        else
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]) : : "memory");
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            o[t] *= corr;
            const u32x4 vf = f8x8_to_f16(x[t].x, x[t].y);
            o[t] = am_mfma(vf, pfh, o[t]);
            o[t] = am_mfma(vf, pfm, o[t]);
            o[t] = am_mfma(vf, pfl, o[t]);
        }
        // the slot's LDS reads are done (lgkmcnt(0) above): refill it with tile j + NBUF
        if (j + NBUF < nl) issue(j + NBUF);
    }
    if (a.stamps && threadIdx.x == 0) a.stamps[blockIdx.x * 4 + 2] = __builtin_amdgcn_s_memrealtime();

    // merge the 4 waves: each publishes (mx, l, o) into its own (drained) image, then wave w merges 16-d tiles
    // t = w, w + 4, ... (dead waves: mx = -inf, l = 0, o = 0)
    float* fo = reinterpret_cast<float*>(wimg);  // [NT][64 lanes][4]
    float* fml = fo + NT * 64 * 4;               // [64] mx, then [64] l
#pragma unroll
    for (int t = 0; t < NT; ++t) *reinterpret_cast<am_float4*>(fo + (t * 64 + lane) * 4) = o[t];
    fml[lane] = mx;
    fml[64 + lane] = l;
    __syncthreads();
    float m4[kAmWaves], w4[kAmWaves], M = -INFINITY;
#pragma unroll
    for (int w = 0; w < kAmWaves; ++w) {
        m4[w] = reinterpret_cast<const float*>(sm + w * WB)[NT * 256 + lane];
        M = fmaxf(M, m4[w]);
    }
    float L = 0.0f;
#pragma unroll
    for (int w = 0; w < kAmWaves; ++w) {
        w4[w] = m4[w] == -INFINITY ? 0.0f : expf(m4[w] - M);
        L = fmaf(w4[w], reinterpret_cast<const float*>(sm + w * WB)[NT * 256 + 64 + lane], L);
    }
    const bool publish = a.defer_merge == 0;
    for (int t = wave; t < NT; t += kAmWaves) {
        am_float4 acc = am_float4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int w = 0; w < kAmWaves; ++w)
            acc += *reinterpret_cast<const am_float4*>(reinterpret_cast<const float*>(sm + w * WB) + (t * 64 + lane) * 4) *
                   w4[w];
        if (i16 < G) {  // lane holds d = 16 t + 4 g + r of q head kvh * G + i16
            const size_t row = ((size_t)(kvh * G + i16) * a.max_splits + wgs) * (HD + kAttnPartPad);
            if (publish) {  // write-through (sc1, 16- and 8-byte stores) for the head's last-arriving workgroup
                const auto rs = __builtin_amdgcn_make_buffer_rsrc(a.part + row, 0, 4u * (HD + kAttnPartPad), 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b128(
                    u32x4{__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]), __float_as_uint(acc[3])},
                    rs, 4u * (t * 16 + 4 * g), 0, 16 /* sc1 */);
                if (t == 0 && g == 0)
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(M), __float_as_uint(L)}, rs, 4u * HD, 0, 16);
            } else {
                float* dst = a.part + row;
                *reinterpret_cast<float4*>(dst + t * 16 + 4 * g) = float4{acc[0], acc[1], acc[2], acc[3]};
                if (t == 0 && g == 0) {
                    dst[HD] = M;
                    dst[HD + 1] = L;
                }
            }
        }
    }
    if (!publish) return;  // partials for the next launch (the kernel boundary publishes them)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains before the arrival
    __syncthreads();
    const int ns = min(pos / ppwg + 1, a.max_splits);  // live workgroups of this kv head
    if (threadIdx.x == 0) {
        const unsigned prev = __hip_atomic_fetch_add(a.counters + kvh, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = prev == (unsigned)(ns - 1);
        if (last) __hip_atomic_store(a.counters + kvh, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (last) {
        if (ns <= 4)
            am_merge<HD, G, 2>(a.part, a.out, kvh, a.max_splits, ns);
        else if (ns <= 8)
            am_merge<HD, G, 4>(a.part, a.out, kvh, a.max_splits, ns);
        else if (ns <= 16)
            am_merge<HD, G, 8>(a.part, a.out, kvh, a.max_splits, ns);
        else
            am_merge<HD, G, 16>(a.part, a.out, kvh, a.max_splits, ns);
        if (a.stamps && threadIdx.x == 0) a.stamps[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memrealtime();
    }
}

}  // namespace sli
