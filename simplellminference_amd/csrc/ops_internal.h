// ops_internal.h — launchers shared between the kernel-level ABI (ops.hip) and the engine (engine.hip).
#pragma once
#include "attention.h"
#include "common.h"

namespace sli {

template <typename KT>
int mha_launch(const float* q, const KT* kc, const KT* vc, float* out, int layer, int pos, const int32_t* pos_dev,
               int T, int hd, int H, int Hkv, long long pos_stride, long long head_stride, long long layer_stride,
               float* part, unsigned* counters, hipStream_t s, int seq_heads = 0, int pos_seq_stride = 0,
               int cache_heads = 0, int defer_merge = 0);

size_t mha_part_bytes(int T, int H, int hd);       // split partials [H][splits][hd + pad], 256-B aligned
size_t mha_workspace_bytes(int T, int H, int hd);  // partials + per-kv-head arrival counters
int attn_wg_positions(int kv_dtype, int head_dim);  // context positions per attention workgroup

int embedding_launch(int token, const int32_t* token_dev, const void* table, int dtype, const float* row_scale,
                     float* out, int vocab, int dim, hipStream_t s);

// sample.h: the argument ranges of sli_sampling (null, or what is wrong), and one draw per row. pd != null: the
// parameters are read from device memory when the kernel runs (pv is ignored).
const char* sample_params_error(const sli_sampling& p);
hipError_t launch_sample(const float* logits, long long row_stride, int rows, int V, const sli_sampling& pv,
                         const sli_sampling* pd, int seq0, const int32_t* pos, int pos_stride, int32_t* out,
                         hipStream_t s);

// gen_sample.h: the per-row sampler. GenRow is what the kernel reads of one sli_gen_params (gen_row: log_min_p is
// computed here, on the host). gen_params_error: the ranges of sli.h (null, or what is wrong); gen_capacity_error: null,
// or why a penalised row cannot take vocabulary V and history rows of hist_len elements. pd != null: `rows` blocks in
// device memory, read when the kernel runs; else pv: `rows` host blocks. table: some row may be penalised.
struct GenRow {
    float temperature;
    int32_t top_k;
    float top_p;
    uint32_t seed;
    float min_p, log_min_p;
    float repetition_penalty, presence_penalty, frequency_penalty;
    int32_t penalty_from;
};
const char* gen_params_error(const sli_gen_params& p);
const char* gen_capacity_error(int V, long long hist_len);
bool gen_penalised(const sli_gen_params& p);
GenRow gen_row(const sli_gen_params& p);
hipError_t launch_sample_gen(const float* logits, long long row_stride, int rows, int V, const GenRow* pv,
                             const GenRow* pd, int seq0, const int32_t* pos, int pos_stride, const int32_t* hist,
                             long long hist_len, bool table, int32_t* out, hipStream_t s);

}  // namespace sli
