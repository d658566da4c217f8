// attn_mfma_f8.h — the FP8 E4M3 K/V cache (SLI_DT_F8E4M3, one byte per element, no scale) as a cache format of the
// MFMA decode attention (attn_mfma.h am_attn): the only attention an FP8 cache runs. The body is the fp16 cache's;
// AmF8 supplies what a cache row's bytes change:
//
//   * a cache row is HD bytes, so a 32-key K + V tile is 8 KiB (hd 128) or 4 KiB (hd 64): half the fp16 cache's
//     bytes per tile, which is why the ring depth goes up to 4 (the same bytes in flight per CU as the fp16
//     cache's 2);
//   * the K operand: a lane reads the 8 codes of its row at d = 32 db + 8 g .. +7 (ds_read_b64) and widens them to
//     the exact fp16 A fragment in registers (common.h f8x8_to_f16); the MFMA stays v_mfma_f32_16x16x32_f16, so q
//     and P keep their three fp16 terms and the arithmetic after the widening is the fp16 cache's;
//   * the V operand: ONE ds_read_b64_tr_b8 per 16-d tile. Per group of 16 lanes it reads a block of 8 rows x 16
//     one-byte columns: lane 2 q + p of the group (q = 0..7, p = 0..1) supplies the address of row q, columns
//     8 p .. 8 p + 7, and lane i receives column i of the 8 rows, row q in its byte q. Lane group g reads rows
//     8 g .. 8 g + 7, so a lane of the Vᵀ A operand holds d = 16 t + i16 of keys 8 g .. 8 g + 7 of the tile;
//   * the key <-> A-row map of the S MFMAs is chosen so that the S accumulators a lane holds are exactly those keys:
//     A row m of S MFMA kt is key 8 (m >> 2) + 4 kt + (m & 3), so lane group g's accumulator r of MFMA kt is key
//     8 g + 4 kt + r, element 4 kt + r of its Pᵀ B operand;
//   * the chunk swizzles are re-derived for the new row length (below).
#pragma once
#include "attn_mfma.h"

namespace sli {

struct AmF8 {
    using KT = f8e4m3;
    static constexpr int EB = 1;       // bytes per element
    static constexpr int MAXBUF = 4;   // ring slots per wave
    static constexpr int VR = 1;       // transposed reads per 16-d tile
    // Chunk swizzles (physical 16-B chunk = logical chunk ^ swizzle(row)). Banks are counted per 32-lane half over the
    // 256-byte bank row, i.e. 16 slots of 16 bytes; a row starts at slot 8 (r & 1) for 128-byte rows and 4 (r & 3) for
    // 64-byte rows.
    //   K: a half-wave's ds_read_b64 touches one logical chunk of the 16 rows 8 a + 4 kt + b (a, b = 0..3), two lanes
    //      per chunk. 128-byte rows: slot 8 (b & 1) + (c ^ swz), so swz takes 8 values over (a, b >> 1); 64-byte rows:
    //      slot 4 b + (c ^ swz), so swz takes 4 values over a.
    //   V: a half-wave's transposed read touches one logical chunk of 16 consecutive rows r. 128-byte rows: slot
    //      8 (r & 1) + (c ^ swz), swz = (r >> 1) & 7; 64-byte rows: slot 4 (r & 3) + (c ^ swz), swz = (r >> 2) & 3.
    __device__ __forceinline__ static int swz_k(int r, int rowb) {
        return rowb == 128 ? (((r >> 3) & 3) << 1) | ((r >> 1) & 1) : (r >> 3) & 3;
    }
    __device__ __forceinline__ static int swz_v(int r, int rowb) { return rowb == 128 ? (r >> 1) & 7 : (r >> 2) & 3; }
    __device__ __forceinline__ static int a_row(int kt, int i16) { return 8 * (i16 >> 2) + 4 * kt + (i16 & 3); }
    __device__ __forceinline__ static int acc_key(int t0, int g, int kt, int r) { return t0 + 8 * g + 4 * kt + r; }
    __device__ __forceinline__ static u32x4 k_frag(const char* krow, int sw, int db, int g) {
        const u32x2 kb = *reinterpret_cast<const u32x2*>(krow + 8 * (g & 1) + ((2 * db + (g >> 1)) ^ sw) * 16);
        return f8x8_to_f16(kb.x, kb.y);
    }
    // this lane's address: row 8 g + (i16 >> 1), 8 bytes at column 8 (i16 & 1) of a 16-d chunk
    template <int NT, int ROWB>
    __device__ __forceinline__ static void v_read(unsigned vbase, int lane, uint2 (&x)[NT * VR]) {
        const int g = lane >> 4, i16 = lane & 15;
        const int vrow = 8 * g + (i16 >> 1), vsw = swz_v(vrow, ROWB);
        const unsigned va = vbase + vrow * ROWB + 8 * (i16 & 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) x[t] = lm_tr8_read(va + ((t ^ vsw) * 16));
    }
    __device__ __forceinline__ static u32x4 v_frag(const uint2* x, int t) { return f8x8_to_f16(x[t].x, x[t].y); }
};

template <int HD, int G, int NBUF>
__global__ void __launch_bounds__(64 * kAmWaves) attn_mfma_f8_kernel(AttnArgs<f8e4m3> a) {
    am_attn<AmF8, HD, G, NBUF>(a);
}

}  // namespace sli
