// kv_copy.h — prefix copy between the sequences of a K/V cache: rows [0, n) of every layer and kv head of sequence
// src to sequence dst (sli_kv_copy_prefix, sli_model_copy_prefix). A cache is [L][B][hkv][T][hd] of 1-, 2- or 4-byte
// elements (FP8 codes, fp16, fp32), K and V apart; the rows [0, n) of one (layer, sequence, kv head) are n * hd
// contiguous elements, so the copy is one run of 16-byte vectors per (layer, kv head, K | V): the kernel knows the
// element size only through the row's bytes.
#pragma once
#include "common.h"

namespace sli {

constexpr int kKcRows = 16;  // rows per workgroup (grid x)

struct KvCopyArgs {
    char* kc;
    char* vc;
    int B, hkv, T;
    int row_bytes;  // hd * element size: >= 64, a multiple of 16
    int src, dst, n;
};

// grid (row blocks of kKcRows, L * hkv * 2): y = (layer * hkv + kv head) * 2 + {0: K, 1: V}
__global__ void __launch_bounds__(256) kv_copy_prefix_kernel(KvCopyArgs a) {
    const int which = blockIdx.y & 1, lh = blockIdx.y >> 1;
    const int layer = lh / a.hkv, head = lh - layer * a.hkv;
    const size_t seq_bytes = (size_t)a.hkv * a.T * a.row_bytes, head_bytes = (size_t)a.T * a.row_bytes;
    char* base = (which ? a.vc : a.kc) + (size_t)layer * a.B * seq_bytes + (size_t)head * head_bytes;
    const uint4* s = reinterpret_cast<const uint4*>(base + (size_t)a.src * seq_bytes);
    uint4* d = reinterpret_cast<uint4*>(base + (size_t)a.dst * seq_bytes);
    const int vpr = a.row_bytes >> 4;  // 16-byte vectors per row
    const int r0 = blockIdx.x * kKcRows;
    const int rows = min(kKcRows, a.n - r0);  // n <= T: the run ends inside this head's rows
    const size_t v0 = (size_t)r0 * vpr;
    for (int i = threadIdx.x; i < rows * vpr; i += blockDim.x) d[v0 + i] = s[v0 + i];
}

// The arguments are the caller's to check (sli_kv_copy_prefix does); n == 0 launches nothing.
static hipError_t launch_kv_copy_prefix(const KvCopyArgs& a, int L, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const dim3 grid((a.n + kKcRows - 1) / kKcRows, L * a.hkv * 2);
    hipLaunchKernelGGL(kv_copy_prefix_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace sli
