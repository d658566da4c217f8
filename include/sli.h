/*
 * sli.h — the C ABI of the MI355X-native decode path (libsli.so).
 *
 * Plain pointers, sizes and status codes only (no torch or HIP types in any signature; a stream is an
 * opaque void* that is a hipStream_t, NULL = the default stream). Device pointers are HIP device
 * memory on the current device. Every entry point returns SLI_OK (0) or an sli_status code; the text
 * of the last error on the calling thread is available from sli_last_error().
 *
 * Two layers:
 *  (1) kernel level — one entry point per reference launcher in include/kernel/cuda/ (*.cuh); the C++
 *      drop-in op:: layer (include/op/, simplellminference_amd/csrc/host/) unpacks mem::Tensor and
 *      calls these;
 *  (2) model level — the whole LlamaModel decode step (source/model/model.cpp:40-187) as one fused,
 *      graph-captured HIP step per token, optionally tensor-parallel over RCCL.
 * Reference citations are /root/reference paths.
 */
#ifndef SLI_H_
#define SLI_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SLI_OK = 0,
    SLI_ERR_ARG = 1,    /* null pointer / bad enum / bad scalar */
    SLI_ERR_SHAPE = 2,  /* tensor dimensions inconsistent (reference: LOG("Tensor with Wrong Dim!")) */
    SLI_ERR_RANGE = 3,  /* token or position out of range (reference: emb_kernel.cpp:10) */
    SLI_ERR_HIP = 4,    /* HIP runtime error */
    SLI_ERR_NOMEM = 5,  /* device allocation failed */
    SLI_ERR_COMM = 6,   /* RCCL error */
    SLI_ERR_STATE = 7,  /* call not valid in the object's current state */
    SLI_ERR_TIMEOUT = 8 /* a host wait on a stream with RCCL collectives made no progress for SLI_COMM_TIMEOUT_MS
                           (default 120 s): a peer or the communicator is wedged; the communicator was aborted */
} sli_status;

/* SLI_DT_MXFP4: OCP microscaling FP4 weights (e2m1 elements, one e8m0 scale per 32 consecutive columns; the layout
 * and the quantisation rule are with sli_quant_mxfp4 below). A weight dtype of the model level and of the
 * sli_*_mxfp4 entry points only.
 * SLI_DT_F8E4M3: OCP FP8 E4M3 ("e4m3fn"), one byte per element and no scale (the format and the quantisation rule
 * are with sli_quant_f8 below). A K/V cache dtype: sli_mha, sli_mha_strided and the sli_*_f8 entry points. */
typedef enum { SLI_DT_F32 = 0, SLI_DT_F16 = 1, SLI_DT_I8 = 2, SLI_DT_MXFP4 = 3, SLI_DT_F8E4M3 = 4 } sli_dtype;

typedef void* sli_stream_t;

int sli_version(void);
const char* sli_status_str(int status);
const char* sli_last_error(void);

/* ---------------------------------------------------------------- device helpers */
int sli_device_count(int* n);
int sli_set_device(int device);
int sli_malloc(void** ptr, size_t bytes);
int sli_free(void* ptr);
int sli_memset(void* ptr, int value, size_t bytes, sli_stream_t stream);
int sli_memcpy_h2d(void* dst, const void* src, size_t bytes, sli_stream_t stream);
int sli_memcpy_d2h(void* dst, const void* src, size_t bytes, sli_stream_t stream);
int sli_memcpy_d2d(void* dst, const void* src, size_t bytes, sli_stream_t stream);
int sli_stream_create(sli_stream_t* out);
int sli_stream_destroy(sli_stream_t stream);
int sli_stream_sync(sli_stream_t stream);

/* ---------------------------------------------------------------- kernel level
 * Each replaces one reference CUDA launcher; semantics follow the reference CPU kernel (the oracle). */

/* kernel::matmul_kernel_cuda (include/kernel/cuda/matmul_kernel.cuh:6-7; CPU semantics
 * source/kernel/cpu/matmul_kernel.cpp:5-28): y[r] = scale * sum_c x[c] * W[r][c]; W row-major
 * [rows][cols] in w_dtype; w_row_scale[rows] multiplies each row for SLI_DT_I8 (NULL otherwise). */
int sli_matmul(const float* x, const void* w, int w_dtype, const float* w_row_scale, float* y, int32_t rows,
               int32_t cols, float scale, sli_stream_t stream);

/* MXFP4 weights. A [rows][cols] tensor needs cols % 32 == 0 and is two arrays in plain OCP layout:
 *   data   uint8 [rows][cols / 2]: element 2i in bits 3:0 of byte i, element 2i + 1 in bits 7:4; a 4-bit code is the
 *          sign in bit 3 and the magnitude {0, .5, 1, 1.5, 2, 3, 4, 6}[bits 2:0];
 *   scales uint8 [rows][cols / 32], e8m0: the block's elements are multiplied by 2^(byte - 127).
 * Quantisation of a block of 32 finite values w (deterministic): amax = max|w|; amax == 0 gives scale byte 127 and
 * codes 0; otherwise e = clamp(floor(log2(amax)) - 2, -127, 127), scale byte e + 127 (255 is never produced), and
 * each |w| * 2^-e (exact) is rounded to the nearest magnitude of the grid, ties to the even code, saturating at 6:
 * <= .25 -> 0, (.25, .75) -> .5, [.75, 1.25] -> 1, (1.25, 1.75) -> 1.5, [1.75, 2.5] -> 2, (2.5, 3.5) -> 3,
 * [3.5, 5] -> 4, > 5 -> 6; the sign bit is w's (a zero may carry either sign). NaN and Inf inputs are out of
 * contract: the result for a block that holds one is unspecified.
 *
 * sli_mxfp4_bytes: the sizes of the two arrays (host only, no device needed); SLI_ERR_SHAPE if cols % 32 != 0.
 * sli_quant_mxfp4: device fp32 [rows][cols] -> data, scales (device; data 16-byte aligned).
 * sli_dequant_mxfp4: the inverse, fp32 [rows][cols] (exact: every element times scale is an fp32 value).
 * sli_matmul_mxfp4: y[r] = scale * sum_c x[c] * W[r][c], x and y fp32, fp32 accumulation, on the GEMV of sli_matmul
 * (x and data 16-byte aligned, cols below 16320). sli_matmul itself rejects SLI_DT_MXFP4 (its row scales are float). */
int sli_mxfp4_bytes(int32_t rows, int32_t cols, size_t* data_bytes, size_t* scale_bytes);
int sli_quant_mxfp4(const float* src, void* data, void* scales, int32_t rows, int32_t cols, sli_stream_t stream);
int sli_dequant_mxfp4(const void* data, const void* scales, float* dst, int32_t rows, int32_t cols,
                      sli_stream_t stream);
int sli_matmul_mxfp4(const float* x, const void* data, const void* scales, float* y, int32_t rows, int32_t cols,
                     float scale, sli_stream_t stream);

/* FP8 E4M3 (SLI_DT_F8E4M3). A byte is 1 sign bit, 4 exponent bits (bias 7) and 3 mantissa bits: exponent field
 * e > 0 is (-1)^s 2^(e - 7) (1 + m / 8), e == 0 the subnormals (-1)^s m 2^-9; the largest finite value is 448
 * (0x7E), there are no infinities, and 0x7F / 0xFF are NaN. Decoding is exact in fp16 and fp32.
 * Quantisation of an fp32 value v (deterministic, the one rule every writer of an FP8 cache shares, common.h
 * f8e4m3_encode): NaN -> 0x7F; otherwise |v| is first clamped to 448 (so every |v| > 448, +-inf included, saturates
 * to +-448 and the NaN codes are never produced from a number), then rounded to the nearest representable value,
 * ties to the even code; the sign bit is v's (-0 -> 0x80). The rule is computed in integer arithmetic, so it does
 * not depend on a hardware convert's saturation or NaN behaviour.
 *
 * sli_quant_f8: device fp32 [n] -> codes uint8 [n]. sli_dequant_f8: the inverse table, fp32 [n] (NaN codes -> NaN). */
int sli_quant_f8(const float* src, void* codes, size_t n, sli_stream_t stream);
int sli_dequant_f8(const void* codes, float* dst, size_t n, sli_stream_t stream);

/* Batched projection for B sequences decoding in lockstep (the reference is batch 1; this serves
 * SURVEY.md §8 config C4): y[b][r] = sum_c x[b][c] * W[r][c] for b < batch <= 8, on MFMA
 * (v_mfma_f32_16x16x32_f16; the fp32 input is carried as fp16 hi + lo columns). x [batch][cols] fp32, W
 * [rows][cols] fp16 (SLI_DT_F16 only), y [batch][rows] fp32, cols % 32 == 0. The workspace
 * (sli_matmul_batch_workspace_bytes, 0 = unsupported shape) holds split-K partials and counters. */
size_t sli_matmul_batch_workspace_bytes(int32_t rows, int32_t cols, int32_t batch);
int sli_matmul_batch(const float* x, const void* w, int w_dtype, float* y, int32_t rows, int32_t cols, int32_t batch,
                     void* workspace, size_t workspace_bytes, sli_stream_t stream);

/* The same projection from int8 weights (per-row symmetric): y[b][r] = (sum_c x[b][c] * W[r][c]) * w_row_scale[r]
 * (NULL scale: 1). W row-major int8 [rows][cols]; the bytes become the MFMA's fp16 A operand exactly in registers,
 * the row scale multiplies the finished fp32 row sum. tiled = 0 streams W as given; tiled = 1 first re-lays W into
 * the model's fragment layout inside the workspace (the tile kernel and row map of the batched model's plain-row
 * projections) and streams that image. Checks and statuses as sli_matmul_batch; the workspace size depends on
 * `tiled` (0 = unsupported shape; no device needed). */
size_t sli_matmul_batch_i8_workspace_bytes(int32_t rows, int32_t cols, int32_t batch, int32_t tiled);
int sli_matmul_batch_i8(const float* x, const void* w, const float* w_row_scale, float* y, int32_t rows, int32_t cols,
                        int32_t batch, int32_t tiled, void* workspace, size_t workspace_bytes, sli_stream_t stream);

/* The same projection from MXFP4 weights (data uint8 [rows][cols / 2] and e8m0 scales uint8 [rows][cols / 32] in the
 * public layout above): y[b][r] = sum_c x[b][c] * code(W[r][c]) * 2^(scale[r][c / 32] - 127). The codes become the
 * MFMA's fp16 A operand exactly and unscaled; each 32-column block's MFMA tile is multiplied by the block's scale in
 * fp32 (the float whose exponent field is the scale byte; byte 0 is the subnormal 2^-127), so no block exponent
 * overflows or flushes an fp16. tiled = 0 streams data and scales as given; tiled = 1 first re-lays both into the
 * model's fragment-layout images inside the workspace and streams those. Checks and statuses as sli_matmul_batch_i8.
 * A plain-rows form of sli_batch_gemm_mxfp4's store role, compiled beside it. */
size_t sli_matmul_batch_mxfp4_workspace_bytes(int32_t rows, int32_t cols, int32_t batch, int32_t tiled);
int sli_matmul_batch_mxfp4(const float* x, const void* data, const void* scales, float* y, int32_t rows, int32_t cols,
                           int32_t batch, int32_t tiled, void* workspace, size_t workspace_bytes, sli_stream_t stream);

/* kernel::rmsnorm_kernel_cuda (rms_kernel.cuh:6-7; CPU rms_kernel.cpp:5-23): y = x / sqrt(mean(x^2)+eps) * w.
 * Single-workgroup reduction: no atomics, no per-call allocation (the reference allocates + memsets a
 * {1} tensor per call and races across blocks, rms_kernel.cu:29-33,48-51). */
int sli_rmsnorm(const float* x, const float* w, float* y, int32_t dim, float eps, sli_stream_t stream);

/* kernel::rope_cache_cal_cuda (rope_kernel.cuh:5-6; CPU rope_kernel.cpp:4-19): the fp32 sin/cos table
 * [max_seq_len][head_dim/2] is computed on the host with libm powf/sinf/cosf (bit-identical to the
 * reference CPU table) and copied to sin_dev / cos_dev. */
int sli_rope_cache(int32_t head_dim, int32_t max_seq_len, float* sin_dev, float* cos_dev, float theta,
                   sli_stream_t stream);

/* kernel::rope_kernel_cuda (rope_kernel.cuh:7-8; CPU rope_kernel.cpp:22-41): rotate-half RoPE of q
 * (q_dim) and k (k_dim) at position pos_dev ? *pos_dev : pos. k is rotated over k_dim only. */
int sli_rope(float* q, float* k, int32_t pos, const int32_t* pos_dev, const float* sin_dev, const float* cos_dev,
             int32_t q_dim, int32_t k_dim, int32_t head_dim, sli_stream_t stream);

/* kernel::mha_kernel_cuda (mha_kernel.cuh:6-21; CPU mha_kernel.cpp:36-77): decode attention for one
 * layer at position pos over a KV cache in REFERENCE layout [L][T][KV] (fp32, fp16 or SLI_DT_F8E4M3).
 * Split-context flash-decoding: needs sli_mha_workspace_bytes() of device scratch, the same for every cache
 * dtype (the reference's {hd,T} score buffer is not needed).
 * An FP8 cache runs the MFMA kernel of attn_mfma_f8.h only (the codes are widened exactly to fp16 in registers, so
 * the arithmetic after the decode is the fp16 cache's): q, both cache bases, the row stride and the head stride
 * must each be a multiple of 16 bytes (SLI_ERR_ARG), head_dim 64 or 128 and n_heads / n_kv_heads in {1, 2, 4, 8}
 * (SLI_ERR_SHAPE). A NaN code in the cache is out of contract there (the kernel reads it as 480).
 * sli_mha_strided: the same attention over ONE layer's cache with explicit strides in elements: position p of kv
 * head h is at k + p * pos_stride + h * head_stride (reference layout: pos_stride = n_kv_heads * head_dim,
 * head_stride = head_dim; the engine's head-major [Hkv][T][hd]: pos_stride = head_dim, head_stride = T * head_dim). */
size_t sli_mha_workspace_bytes(int32_t max_seq_len, int32_t n_heads, int32_t head_dim);
int sli_mha(const float* q, const void* kcache, const void* vcache, int kv_dtype, float* out, int32_t layer,
            int32_t pos, int32_t max_seq_len, int32_t head_dim, int32_t n_heads, int32_t n_kv_heads,
            void* workspace, size_t workspace_bytes, sli_stream_t stream);
int sli_mha_strided(const float* q, const void* k, const void* v, int kv_dtype, float* out, int32_t pos,
                    int32_t max_seq_len, int32_t head_dim, int32_t n_heads, int32_t n_kv_heads, int64_t pos_stride,
                    int64_t head_stride, void* workspace, size_t workspace_bytes, sli_stream_t stream);

/* softmax_kernel_cpu (mha_kernel.cpp:7-20) as a standalone in-place op over n floats. */
int sli_softmax(float* x, int32_t n, sli_stream_t stream);

/* kernel::swiglu_kernel_cuda (swiglu_kernel.cuh:5; CPU swiglu_kernel.cpp:5-15): out = sigmoid(gate)*up
 * (the reference variant; see sli_model_config.act_mode for SiLU). */
int sli_swiglu(const float* up, const float* gate, float* out, int32_t n, sli_stream_t stream);

/* kernel::add_kernel_cuda (add_kernel.cuh:6; CPU add_kernel.cpp:5-14): out = a + b. */
int sli_add(const float* a, const float* b, float* out, int32_t n, sli_stream_t stream);

/* kernel::emb_kernel_cuda (emb_kernel.cuh:6-7; CPU emb_kernel.cpp:4-21): out = table[token] (row
 * dequantised for SLI_DT_I8 with row_scale). token = token_dev ? *token_dev : token. Returns
 * SLI_ERR_RANGE for a host token outside [0, vocab). A device token cannot be checked without a host
 * sync: outside [0, vocab) it fills `out` with quiet NaNs, so the failure (the reference's LOG-exit,
 * emb_kernel.cu:15-16) propagates loudly instead of as a plausible zero embedding. */
int sli_embedding(int32_t token, const int32_t* token_dev, const void* table, int dtype, const float* row_scale,
                  float* out, int32_t vocab, int32_t dim, sli_stream_t stream);

/* argmaxLayer::forward (source/op/argmax.cpp:7-17) on device: first index of the maximum. */
int sli_argmax(const float* logits, int32_t n, int32_t* out_dev, sli_stream_t stream);

/* Seeded temperature / top-k / top-p sampling (no reference counterpart: model.cpp:157-183 decodes greedily). The
 * rule, for one row of fp32 logits l[0..V), the parameters below, a sequence id s and a position pos:
 *  - Candidates. NaN and -inf logits are never candidates. If the row has no finite maximum (every logit NaN or -inf,
 *    or a +inf present) the result is sli_argmax's for the row and nothing below applies.
 *  - Top-k. top_k <= 0 or top_k >= V: off. Otherwise tau_k is the k-th largest logit counted with multiplicity (a NaN
 *    counts as -inf) and C_k = {i : l_i >= tau_k}: ties at the boundary are all kept. The comparison is on the fp32
 *    values, so -0 equals +0. The set is exact.
 *  - Top-p over C_k. top_p = 1: off. Otherwise q_i = exp((l_i - m) / T) / Z with m the maximum and Z the sum over
 *    C_k; tau_p is the largest logit value v with sum{q_i : i in C_k, l_i >= v} >= top_p, and C = {i in C_k :
 *    l_i >= tau_p}: ties are kept. (Computed with fp32 exp and exact integer sums, csrc/sample.h: the set can differ
 *    from an exact evaluation only where a cumulative mass lies within about 1e-5 of top_p.)
 *  - The draw, Gumbel-max. h_i = sli_rng_u32(seed, (SLI_SAMPLE_STREAM << 16) | (s & 0xFFFF), ((uint64)pos << 32) | i)
 *    (sli_synth.h); u_i = (2 (h_i >> 9) + 1) 2^-24, exact in fp32 and never 0 or 1; key_i = l_i / T - log(-log(u_i))
 *    in fp32 (IEEE divide and subtract, the accurate logf). The token is the index of the largest key over C, the
 *    first index among equal keys.
 *  - The counter of the draw is the position, not a running count: the same (seed, s, pos, logits) always gives the
 *    same token, bit for bit from run to run.
 * temperature in [1e-2, 1e2], top_p in (0, 1], top_k >= 0; anything else (a NaN included) is SLI_ERR_ARG, decided
 * before the device is touched. */
typedef struct {
    float temperature;
    int32_t top_k;
    float top_p;
    uint32_t seed;
} sli_sampling;
enum { SLI_SAMPLE_STREAM = 12 }; /* the draw's stream kind, after sli_synth.h's tensor streams (1 .. 11) */

/* One draw per row: out_dev[r] = the token of row r (logits + r * row_stride, `vocab` floats) drawn as sequence
 * seq0 + r at position pos_dev[r * pos_stride]. The positions are read on the device, so the call is graph-capturable
 * like sli_embedding. row_stride >= vocab, or 0: `rows` independent draws from one distribution. One launch of one
 * workgroup per row, whose only scratch is LDS, so there is no workspace. `p` is a host pointer. pos_stride >= 0. */
int sli_sample(const float* logits, int64_t row_stride, int32_t rows, int32_t vocab, const sli_sampling* p,
               int32_t seq0, const int32_t* pos_dev, int32_t pos_stride, int32_t* out_dev, sli_stream_t stream);

/* Per-row generation parameters (no reference counterpart): sli_sample's rule with a block of its own per row, token
 * penalties before it and min-p after it. The rule, for one row of fp32 logits l[0..V), a block P, a history h (the
 * sequence's tokens by position) and a position pos:
 *  - Penalties. Active iff repetition_penalty != 1 or presence_penalty != 0 or frequency_penalty != 0. n_i = #{j :
 *    penalty_from <= j <= pos, h[j] == i}; a history entry outside [0, V) is not counted, and no address is ever formed
 *    from it; penalty_from > pos counts nothing. For n_i > 0: a = l_i > 0 ? l_i / repetition_penalty : l_i *
 *    repetition_penalty; b = a - presence_penalty; l'_i = b - frequency_penalty * (float)n_i, each operation one IEEE
 *    fp32 operation rounded to nearest, with no contraction. For n_i == 0, l'_i is l_i bit for bit. Inactive: l' = l
 *    and the history is not read. A NaN stays NaN; +-inf follow IEEE.
 *  - Greedy row. temperature == 0: the token is sli_argmax's answer for l' (first maximum, its NaN and +-0 semantics),
 *    and nothing below applies.
 *  - Sampled row. sli_sample's rule, word for word, on l' with (temperature, top_k, top_p, seed), the sequence id and
 *    pos gives the candidate set C; a row with no finite maximum gives sli_argmax(l'). Then min-p: min_p == 0 is off;
 *    otherwise c = (float)log((double)min_p), computed on the host, m' is the maximum of l' and C_m = {i : (l'_i - m')
 *    / T >= c} with an IEEE fp32 subtract and divide. The Gumbel-max draw runs over the intersection of C and C_m,
 *    which is never empty: the maximum is in both. With every new field neutral the token is bit-identical to
 *    sli_sample's.
 * Ranges (anything else, a NaN included, is SLI_ERR_ARG before the device is touched): temperature 0 or in [1e-2,
 * 1e2]; top_k >= 0; top_p in (0, 1]; min_p in [0, 1); repetition_penalty in [0.1, 10]; presence_penalty and
 * frequency_penalty in [-100, 100]; penalty_from >= 0; n_stop in [0, 8]; max_pos >= 0. */
enum { SLI_MAX_STOP = 8 };
typedef struct {
    float temperature; int32_t top_k; float top_p; uint32_t seed;         /* sli_sampling's four; temperature 0: greedy */
    float min_p, repetition_penalty, presence_penalty, frequency_penalty; /* 0, 1, 0, 0: off */
    int32_t penalty_from;                                                 /* first history position counted */
    int32_t max_pos;                                                      /* 0: none (model level only) */
    int32_t n_stop; int32_t stop[SLI_MAX_STOP];                           /* model level only */
} sli_gen_params;

/* sli_sample with a host array of `rows` blocks, one per row, and the rows' histories: row r reads hist_dev + r *
 * hist_stride (int32 tokens by position, hist_stride elements: a position at or past hist_stride is not read).
 * hist_dev may be NULL iff no row has an active penalty, otherwise SLI_ERR_ARG; hist_stride >= 1 then. stop and
 * max_pos are ignored here. out_dev[r] is -1 for a row with temperature 0 and no active penalty: such a row needs
 * nothing from the sampler (its token is sli_argmax's), and its workgroup leaves at once. One workgroup per row, so a
 * row's token does not depend on the other rows of the call, and it is bitwise reproducible: every sum is an integer
 * (csrc/gen_sample.h). Rows without an active penalty never touch the history. Graph-capturable like sli_sample;
 * the blocks are read during the call. Capacity (SLI_ERR_SHAPE beyond it, with the numbers; only where a row is
 * penalised): vocab <= 262144 and hist_stride <= 4097, the workgroup's LDS bitmap and count table. */
int sli_sample_gen(const float* logits, int64_t row_stride, int32_t rows, int32_t vocab, const sli_gen_params* p,
                   int32_t seq0, const int32_t* pos_dev, int32_t pos_stride, const int32_t* hist_dev,
                   int64_t hist_stride, int32_t* out_dev, sli_stream_t stream);

/* Scoring (no reference counterpart). The rule, for one row of V fp32 logits l and a target t:
 *   lse = M + log(sum_j exp(l_j - M)) with M = max_j l_j;  logprob = l_t - lse;
 *   top = the first index of the maximum in sli_argmax's order (-0 equals +0; a NaN never displaces the best so far,
 *   a NaN at index 0 is never displaced);  top_logprob = l_top - lse.
 * All of it in fp32, in a fixed summation order (csrc/score.h). -inf logits contribute 0. A target outside [0, V)
 * gives logprob = NaN, and no address is ever formed from it. A row with a NaN logit gives NaN log-probabilities.
 * The results are bitwise reproducible from run to run, and a row's result does not depend on the other rows of the
 * launch: fixed-order merges, no floating-point atomics.
 * sli_score_rows: M rows at logits + m * ld (ld >= V, ld % 4 == 0, logits 16-byte aligned; columns V .. ld - 1 are
 * never used), targets int32 [M] on the device; logprob [M], top [M] and top_logprob [M] on the device, the last two
 * nullable. One workgroup per row and one read of the rows: the launch is bound by M * V * 4 bytes. Bad arguments are
 * SLI_ERR_ARG before the device is touched. */
int sli_score_rows(const float* logits, int32_t M, int32_t V, int32_t ld, const int32_t* targets, float* logprob,
                   int32_t* top, float* top_logprob, sli_stream_t stream);

/* ---------------------------------------------------------------- model level */
typedef struct {
    int32_t vocab, dim, n_heads, n_kv_heads, head_dim, ffn, n_layers, max_len;
    float eps, theta;
    int32_t w_dtype;  /* SLI_DT_F32 / SLI_DT_F16 / SLI_DT_I8 (per-row symmetric; any batch) / SLI_DT_MXFP4 (fp32 weights handed to
                         the model are quantised by the rule at sli_quant_mxfp4; batch 1, or batch <= 8 for a model
                         created with SLI_CREATE_MX_BATCH; the launch graph only; dim, the local ffn width and the local q width multiples of 32, else
                         SLI_ERR_SHAPE) */
    int32_t kv_dtype; /* SLI_DT_F32 / SLI_DT_F16 / SLI_DT_F8E4M3 (one byte per element, the rule at sli_quant_f8; with
                         fp16 and int8 weights at any batch, MXFP4 at batch 1 or batch <= 8 under SLI_CREATE_MX_BATCH, not fp32 weights: SLI_ERR_ARG; the launch
                         graph only; prompts through the decode step, or through the GEMM prefill after
                         sli_model_set_prefill(SLI_PREFILL_GEMM_KV8); sli_model_get_kv returns the decoded fp32) */
    int32_t act_mode; /* 0: reference sigmoid(gate)*up (swiglu_kernel.cpp:12-13); 1: SiLU(gate)*up */
    int32_t tp_rank, tp_size;
    int32_t device;
    int32_t batch;    /* sequences decoding in lockstep, <= 8 (0 or 1: batch 1, the reference's case).
                         batch > 1 runs the projections on MFMA (sli_matmul_batch, sli_matmul_batch_i8,
                         sli_matmul_batch_mxfp4) and needs fp16 or int8 weights, or MXFP4 weights and
                         SLI_CREATE_MX_BATCH (sli_model_create_flags) */
} sli_model_config;

typedef struct sli_model sli_model;

/* Tensor-parallel shard plan (host only, no device needed): the window of the full reference-layout
 * tensor `kind` (sli_synth.h) that rank cfg->tp_rank holds, and where it lands in the rank's fused
 * buffer. Megatron split: wq/wk/wv/gate/up by output rows (heads / FFN columns),
 * wo/down by input columns, embedding and norms replicated, LM head = embedding rows [vocab_lo,
 * vocab_lo + vocab_n). */
typedef struct {
    int32_t row_lo, n_rows, col_lo, n_cols, full_cols;
    int32_t dst_row_off; /* first row inside the rank's fused buffer ([q;k;v] or [gate;up]) */
} sli_shard_window;
int sli_tp_plan(const sli_model_config* cfg, int32_t kind, sli_shard_window* out);
int sli_tp_vocab(const sli_model_config* cfg, int32_t* vocab_lo, int32_t* vocab_n);

/* One-shot all-reduce over xGMI (replaces the step's RCCL all-reduces; one process per GPU): every rank
 * exports its comm buffer (uncached device memory) with sli_model_comm_handle, the ranks exchange the
 * handles over any host transport, each opens all of them with sli_model_comm_open (handles [nranks][
 * sli_model_comm_handle_bytes()] in rank order) and switches with sli_model_set_allreduce. Each call
 * pushes the rank's partial to every rank, raises a flag per rank, waits (bounded) for all flags and
 * sums in rank order, so every rank holds bit-identical x; the argmax keys use the same exchange.
 * SLI_ALLREDUCE_FUSED (batch 1): the same exchange inside the wo / down GEMV launches — their epilogues
 * push the finished rows into the peers' slots and the launch's last workgroup waits and sums (no
 * separate all-reduce launch).
 * SLI_ALLREDUCE_FUSED_WG (ranks on distinct devices, any batch): the fused exchange per workgroup — workgroup w
 * (batch > 1: MFMA group g) of every rank owns the same rows, waits for the same workgroup of the peers and
 * sums its own rows (no launch-wide arrival, no single summing workgroup). Every workgroup waits, so ranks
 * sharing one device would starve each other of CUs unless their grids fit together
 * (SLI_DEBUG_GEMV_MAX_BLOCKS). The separate ONESHOT sum is sliced over workgroups the same way. */
enum { SLI_ALLREDUCE_RCCL = 0, SLI_ALLREDUCE_ONESHOT = 1, SLI_ALLREDUCE_FUSED = 2, SLI_ALLREDUCE_FUSED_WG = 3 };
int sli_model_comm_handle_bytes(void);
int sli_model_comm_handle(sli_model* m, void* out, int32_t n);
int sli_model_comm_open(sli_model* m, const void* handles, int32_t nranks);
int sli_model_set_allreduce(sli_model* m, int32_t mode);
/* RCCL unique id for tensor parallelism (broadcast it from rank 0 with any host transport). */
int sli_comm_id_bytes(void);
int sli_comm_get_id(void* out);

int sli_model_create(const sli_model_config* cfg, const void* comm_id, sli_model** out);
/* sli_model_create with creation flags; flags = 0 is sli_model_create exactly. An unknown bit is SLI_ERR_ARG, decided
 * before the device is touched.
 * SLI_CREATE_MX_BATCH: an SLI_DT_MXFP4 model may have batch > 1 (<= 8): its projections run on MFMA from FP4 tiles
 * (bgemm.h), with every cache type. Without the flag that combination is refused as before. It has no effect on
 * fp32, fp16 and int8 models (fp32 weights at batch > 1 stay refused). The limits of every batched model hold: the
 * launch graph only, prompts through the decode step, dim <= 4096, projection inputs multiples of 32. */
enum { SLI_CREATE_MX_BATCH = 1 };
int sli_model_create_flags(const sli_model_config* cfg, const void* comm_id, uint32_t flags, sli_model** out);
int sli_model_destroy(sli_model* m);
/* Seeded synthetic weights (include/sli_synth.h), generated on device in this rank's shard. */
int sli_model_init_synthetic(sli_model* m, uint32_t seed);
/* Place one full, unsharded, reference-layout fp32 tensor (kind/index from sli_synth.h). */
int sli_model_set_weight(sli_model* m, int32_t kind, int32_t index, const float* host, int64_t n);
/* Load the reference's flat fp32 weight file (model.cpp:204-245 read, :336-469 layout). */
int sli_model_load_flat(sli_model* m, const char* path);
/* Zero the KV cache and the decode state. */
int sli_model_reset(sli_model* m);
/* Fill K/V rows [0, upto) of every layer with the synthetic N(0,1) values (bench context fill); sequence b
 * of a batch uses seed + b. */
int sli_model_fill_kv_synthetic(sli_model* m, uint32_t seed, int32_t upto);
/* Decode state: the token fed at position pos. advance=1: after each step pos += 1 and the next token
 * is the teacher-forced prompt id or the greedy argmax (model.cpp:157-183); advance=0: the step is
 * idempotent (recomputes the same position; the bench mode). */
int sli_model_set_state(sli_model* m, int32_t token, int32_t pos, int32_t advance);
int sli_model_set_prompt(sli_model* m, const int32_t* ids, int32_t n);
int sli_model_get_state(sli_model* m, int32_t* pos, int32_t* token, int32_t* last_argmax, int32_t* error);
/* Per-sequence forms for batch > 1 (seq < batch). The sequence-less setters above act on every sequence,
 * the getters on sequence 0. */
int sli_model_set_state_seq(sli_model* m, int32_t seq, int32_t token, int32_t pos, int32_t advance);
int sli_model_set_prompt_seq(sli_model* m, int32_t seq, const int32_t* ids, int32_t n);
int sli_model_get_state_seq(sli_model* m, int32_t seq, int32_t* pos, int32_t* token, int32_t* last_argmax,
                            int32_t* error);
/* Prompt prefill (batch-1 models): positions 0 .. n-2 of the prompt run through the layers in chunks of up
 * to 256 positions, every projection one MFMA GEMM over the chunk and attention block-causal over the
 * cache (fp16 / int8 weights, MXFP4 after sli_model_set_prefill(SLI_PREFILL_GEMM), an FP8 K/V cache after
 * sli_model_set_prefill(SLI_PREFILL_GEMM_KV8), head_dim 64 / 128; otherwise
 * through the decode step, teacher-forced; under
 * multi-process tensor parallelism every rank calls it, the chunk's residual rows all-reduced over RCCL
 * twice per layer), filling the K/V cache; the state is left at
 * (token ids[n-1], position n-1, advancing, prompt = ids), so the next sli_model_step yields the first
 * greedy token exactly as the reference's token-by-token predict (model.cpp:157-165) would. A prompt is a
 * continuation whose start is 0: behind its own argument checks this is sli_model_extend(m, ids, 0, n), on a
 * fresh model and on one that holds another prompt and has stepped alike. */
int sli_model_prefill(sli_model* m, const int32_t* ids, int32_t n);
/* Which path sli_model_prefill takes for this model: 1 = chunked MFMA GEMMs (prefill.h), 0 = the decode step,
 * teacher-forced (fp32 weights, batch > 1, unsupported shapes, a TP rank without an RCCL communicator, or an FP8 K/V
 * cache under any mode but SLI_PREFILL_GEMM_KV8). */
int sli_model_prefill_path(const sli_model* m);
/* Which path the next prefill takes. SLI_PREFILL_AUTO (the default): the GEMM prefill where the model can take it,
 * except MXFP4 weights, which stay on the decode step; SLI_PREFILL_GEMM: the chunked MFMA prefill for every weight
 * type that has one (fp16, int8, MXFP4), SLI_ERR_STATE with the reason where the model cannot take it (fp32 weights,
 * an FP8 K/V cache, batch > 1, a TP rank without a communicator, unsupported shapes); SLI_PREFILL_DECODE: the teacher-forced decode
 * step for any model; SLI_PREFILL_GEMM_KV8: SLI_PREFILL_GEMM for every model, and also accepted by a model with an
 * FP8 E4M3 K/V cache that otherwise qualifies (the chunk's K/V rows are quantised in the q/k/v GEMM's epilogue and the
 * chunk attention reads the codes; under the other three modes an FP8-cache model keeps the decode step, and
 * SLI_PREFILL_GEMM its refusal). May be changed between prefills; sli_model_prefill_path reports the outcome. The
 * ranks of an in-process group are set through sli_tp_group_set_prefill. */
enum { SLI_PREFILL_AUTO = 0, SLI_PREFILL_GEMM = 1, SLI_PREFILL_DECODE = 2, SLI_PREFILL_GEMM_KV8 = 3 };
int sli_model_set_prefill(sli_model* m, int32_t mode);
/* 1: the batch-1 decode step runs each layer's q/k/v projection and attention as ONE launch (qkv_attn.h: the
 * attention's K/V rows below the position stream while the projection runs; q and this step's K/V row are
 * handed over inside the launch); 0: separate launches (model.cpp:70-84's matmul / rope / mha sequence either
 * way).
 * Taken where the shape qualifies (heads per kv head 1 or 2, head_dim 64 / 128, fp16 K/V cache, fp16 / int8
 * weights, an attention grid of at most a quarter of the CUs) and SLI_QKV_ATTN allows it
 * (1: always; 0: never; unset: single-rank models). */
int sli_model_fused_qkv_attn(sli_model* m);
/* sli_model_predict with the prompt prefilled: tokens_out[t] as sli_model_predict; logits_out rows for
 * positions < n_prompt - 1 (not computed by the prefill) are NaN. */
int sli_model_predict_prefill(sli_model* m, const int32_t* prompt, int32_t n_prompt, int32_t max_length,
                              int32_t* tokens_out, float* logits_out);
/* Packed prompt prefill for batched models, and per-sequence admission.
 *
 * The packing rule (host only, no device is touched). Sequence seqs[i] with a prompt of lens[i] tokens contributes
 * rows for its positions 0 .. lens[i]-2 (the last prompt token runs as an ordinary decode step), cut into groups of 16
 * positions aligned on the sequence's own positions (p0 % 16 == 0), the last with nv = (lens[i]-1) % 16 valid rows, or
 * 16 when that is zero; a length of 1 contributes nothing. The groups of the listed sequences are concatenated in list
 * order, each sequence's in ascending position; chunks are consecutive runs of 16 groups (256 rows); the last chunk
 * takes the smallest of 32 / 64 / 128 / 256 rows that holds its groups and is padded with groups of nv == 0, which
 * compute and write nothing to the cache (they name the last real group's sequence at p0 = 0).
 * groups receives the groups of all chunks, padding included (chunk c's start at 16 * c), chunk_rows each chunk's rows,
 * *n_chunks their number. SLI_ERR_RANGE for a buffer that is too small and for lens[i] < 1. */
typedef struct {
    int32_t seq, p0, nv; /* 16 chunk rows: positions p0 .. p0+15 of sequence seq, the first nv valid */
} sli_pf_group;
int sli_prefill_pack(const int32_t* seqs, const int32_t* lens, int32_t n_seqs, sli_pf_group* groups, int32_t cap_groups,
                     int32_t* chunk_rows, int32_t cap_chunks, int32_t* n_chunks);
/* Prefill the listed sequences (distinct, < batch; prompts [n_seqs][ld], lens[i] tokens of row i) of a model of any
 * batch 1 .. 8 with their own prompts: chunks packed by the rule above run through the layers as the MFMA GEMMs of
 * sli_model_prefill, the embedding, the q/k/v epilogue and the chunk attention reading the device-resident group table
 * (prefill.h PfSegs) that sli_model_prefill's chunks read too, there with one sequence's groups. Every other
 * sequence's cache rows, state, prompt and history are untouched, so a finished sequence can be replaced inside a running batch. Afterwards sequence seqs[i] is at
 * (token ids[n-1], position n-1, advancing, prompt = ids) and its history holds ids. Prompts are teacher-forced: the
 * sampling state is not consulted. Takes fp16 / int8 / MXFP4 weights (MXFP4 at batch > 1: SLI_CREATE_MX_BATCH) with an
 * fp16 or FP8 E4M3 cache, head_dim 64 / 128, projection depths that are multiples of 64, a single rank; it is not bound
 * by sli_model_set_prefill, whose modes it ignores. SLI_ERR_STATE with the reason for fp32 weights, an fp32 cache,
 * tp_size > 1, ranks of an in-process group and unsupported shapes (no fallback). Argument errors are decided before
 * any state or device memory is touched: a duplicate or out-of-range sequence is SLI_ERR_ARG, a length outside
 * [1, min(ld, max_len)] or a token outside the vocabulary SLI_ERR_RANGE. Behind these checks the call is
 * sli_model_extend_seqs with every start 0, counts = lens and advance 1: one host driver serves both. */
int sli_model_prefill_seqs(sli_model* m, const int32_t* seqs, int32_t n_seqs, const int32_t* prompts,
                           const int32_t* lens, int32_t ld);
int sli_model_prefill_seqs_ok(const sli_model* m); /* 1: the model takes sli_model_prefill_seqs */
/* Test hook (no device needed): the argument checks of sli_model_prefill_seqs and sli_model_score_seqs, in their order,
 * as a model of `batch` sequences, max_len `max_len` and `vocab` tokens makes them. */
int sli_debug_prefill_seqs_args(int32_t batch, int32_t max_len, int32_t vocab, const int32_t* seqs, int32_t n_seqs,
                                const int32_t* prompts, const int32_t* lens, int32_t ld);
/* Score prompts: sli_model_prefill_seqs, and the log-probability of every prompt token given the tokens before it (the
 * rule at sli_score_rows). The same arguments, the same checks in the same order, the same refusals, the same packing;
 * the K/V rows, state, prompt and history it leaves are bit for bit those of sli_model_prefill_seqs, every unlisted
 * sequence untouched. After each chunk's last layer the chunk's rows run through the final RMSNorm, the LM head (the
 * embedding table in the model's weight format: one GEMM over the chunk, role 3 of sli_prefill_gemm) and one
 * sli_score_rows-style launch that reads the group table: the hidden state of position t scores token t + 1.
 * Outputs are host arrays [n_seqs][ld]: entry (i, t), 1 <= t < lens[i], is about prompts[i][t]; entry (i, 0) and the
 * entries at t >= lens[i] are NaN / -1 / NaN. top and top_logprob may be NULL. A prompt of length 1 scores nothing.
 * The scoring chunks are captured graphs of their own, so sli_model_prefill_seqs replays what it always did. The
 * logits chunk ([256][vocab rounded up to 4] fp32: 131 MB at a vocabulary of 128 256) and the result buffers are
 * allocated at the first call and freed with the model; a failed allocation is SLI_ERR_NOMEM and touches no sequence.
 * The sampling state is not consulted. Batch 1 .. 8, fp16 / int8 / MXFP4 weights, an fp16 or FP8 cache; a single
 * rank only: under tensor parallelism the logits are vocab-sharded, so tp_size > 1 and the ranks of an in-process
 * group are SLI_ERR_STATE with that reason. */
int sli_model_score_seqs(sli_model* m, const int32_t* seqs, int32_t n_seqs, const int32_t* prompts,
                         const int32_t* lens, int32_t ld, float* logprob, int32_t* top, float* top_logprob);
int sli_model_score_seqs_ok(const sli_model* m); /* 1: the model takes sli_model_score_seqs */
/* sli_model_predict_batch with every prompt prefilled (sli_model_prefill_seqs over all `batch` sequences), then
 * max_length - min(lens) + 1 steps; sequence b waits at its last prompt position (idempotent steps) for the first
 * lens[b] - min(lens) of them, so all sequences finish together at position max_length. max(lens) <= max_length <=
 * max_len. tokens_out[b][t] as sli_model_predict_batch; logits_out [max_length][batch][local vocab] holds at (t, b) the
 * logits of the step that fed position t, NaN for t < lens[b] - 1. */
int sli_model_predict_batch_prefill(sli_model* m, const int32_t* prompts, const int32_t* lens, int32_t ld,
                                    int32_t max_length, int32_t* tokens_out, float* logits_out);
/* Continuing sequences: prefill and score from a start position.
 *
 * The packing rule with a start (host only). Sequence seqs[i] contributes rows for its positions starts[i] ..
 * starts[i] + counts[i] - 2 (its last token is left for an ordinary decode step). Its first group runs from the start
 * to the next 16-boundary of its own positions: {seq, s, min(16 - s % 16, counts[i] - 1)}; every later group is aligned
 * (p0 % 16 == 0) as in sli_prefill_pack; a count of 1 contributes nothing. Concatenation in list order, 16 groups to a
 * chunk, the last chunk's size bucket and the padding groups are sli_prefill_pack's, and with every start 0 and counts =
 * lens the output is sli_prefill_pack's entry for entry (one planner serves both). A row at or past the first boundary
 * keeps the group-mates it has in the from-zero plan; a row of a partial first group only meets key tiles that are
 * masked for it. SLI_ERR_RANGE for a buffer that is too small, a count below 1, a start below 0. */
int sli_prefill_pack_from(const int32_t* seqs, const int32_t* starts, const int32_t* counts, int32_t n_seqs,
                          sli_pf_group* groups, int32_t cap_groups, int32_t* chunk_rows, int32_t cap_chunks,
                          int32_t* n_chunks);
/* Extend the listed sequences of a model of batch 1 .. 8 from a start position each: tokens is [n_seqs][ld], tokens[i][j]
 * the token at position starts[i] + j, counts[i] of them; starts == NULL means each sequence's current position. Rows
 * [0, pos_i) of a sequence's cache are taken as valid, pos_i its state position (a fresh or reset sequence: 0). The
 * chunks, packed by the rule above, replay the graphs sli_model_prefill_seqs captured (one per chunk size); the same
 * models, the same SLI_ERR_STATE refusals, sli_model_set_prefill ignored. Afterwards sequence seqs[i] is at (token
 * tokens[i][counts[i]-1], position starts[i] + counts[i] - 1), n_forced = starts[i] + counts[i]; its prompt and history
 * hold the tokens at [start, start + count), history below the start is kept; cache rows below the start and every
 * unlisted sequence's rows, state, prompt and history are untouched. advance == 1 leaves the sequences advancing, as
 * sli_model_prefill_seqs does; advance == 0 leaves them waiting (idempotent steps) while the rest of the batch steps: a
 * partly admitted prompt. A start below the position is a rollback: rows from the start on are overwritten as they are
 * recomputed, rows past the new end stay stale and are never read. sli_model_prefill_seqs is the case of every start 0
 * (and sli_model_score_seqs that of sli_model_score_extend_seqs): the prompt calls run this call's driver behind their
 * own checks, so a call with every start 0 leaves what they leave bit for bit.
 * The arguments are judged before any state or device memory is touched, each condition over every listed sequence
 * before the next: n_seqs outside [1, batch], a sequence out of range or listed twice: SLI_ERR_ARG; then SLI_ERR_RANGE
 * for counts[i] outside [1, ld]; starts[i] + counts[i] > max_len; a token outside the vocabulary; starts[i] outside
 * [0, pos_i]. */
int sli_model_extend_seqs(sli_model* m, const int32_t* seqs, int32_t n_seqs, const int32_t* tokens,
                          const int32_t* starts, const int32_t* counts, int32_t ld, int32_t advance);
/* sli_model_extend_seqs through the scoring graphs of sli_model_score_seqs (the same models as that call). Outputs are
 * host arrays [n_seqs][ld]: entry (i, j), 1 <= j < counts[i], is about tokens[i][j] given everything before it; entry
 * (i, 0) and the entries at j >= counts[i] are NaN / -1 / NaN. top and top_logprob may be NULL. What it leaves behind
 * is bit for bit what sli_model_extend_seqs leaves. */
int sli_model_score_extend_seqs(sli_model* m, const int32_t* seqs, int32_t n_seqs, const int32_t* tokens,
                                const int32_t* starts, const int32_t* counts, int32_t ld, int32_t advance,
                                float* logprob, int32_t* top, float* top_logprob);
/* The one-sequence route of a batch-1 model, beside sli_model_prefill: tokens[j] is the token at position start + j
 * (start == -1: the current position), the checks of sli_model_extend_seqs in their order. It follows
 * sli_model_set_prefill as sli_model_prefill does: on the GEMM path the group table is filled by the rule above,
 * otherwise the tokens are teacher-forced through the decode step from the start. An fp32 K/V cache always continues
 * through the decode step when start > 0 (its chunk attention takes consecutive 64-row blocks only). The sequence is left
 * advancing at its last token. */
int sli_model_extend(sli_model* m, const int32_t* tokens, int32_t start, int32_t count);
/* Test hook (no device needed): the argument checks of the extend calls, in their order, as a model of `batch`
 * sequences standing at pos[0 .. batch), max_len `max_len` and `vocab` tokens makes them. starts may be NULL. */
int sli_debug_extend_seqs_args(int32_t batch, int32_t max_len, int32_t vocab, const int32_t* pos, const int32_t* seqs,
                               int32_t n_seqs, const int32_t* tokens, const int32_t* starts, const int32_t* counts,
                               int32_t ld);
/* Prefix copy between sequences (csrc/kv_copy.h): K and V rows [0, n) of every layer and kv head from sequence src to
 * sequence dst, one launch of 16-byte vector copies on the stream. kc / vc: [L][B][hkv][T][hd] of elem_bytes (1, 2 or
 * 4) bytes per element, 16-byte aligned; a row (hd * elem_bytes) at least 64 bytes and a multiple of 16; src != dst,
 * both < B; 0 <= n <= T (0: nothing is launched). Every other byte of both caches is untouched. */
int sli_kv_copy_prefix(void* kc, void* vc, int32_t elem_bytes, int32_t L, int32_t B, int32_t hkv, int32_t T, int32_t hd,
                       int32_t src, int32_t dst, int32_t n, sli_stream_t stream);
/* The same on a model's own cache, with history [0, n]: src != dst (SLI_ERR_ARG), 0 <= n <= src's position
 * (SLI_ERR_RANGE). dst is left waiting at (src's token at position n, position n, not advancing), so it can be extended
 * from any start <= n; src and every other sequence are untouched. */
int sli_model_copy_prefix(sli_model* m, int32_t src, int32_t dst, int32_t n);
/* The tokens fed at positions [0, n) of sequence seq. */
int sli_model_get_history(sli_model* m, int32_t seq, int32_t n, int32_t* out);
/* Execution of the step: SLI_EXEC_LAUNCHES, one hipGraph of ~5 fused launches per layer (every configuration);
 * SLI_EXEC_PERSIST, the embedding, then EVERY layer as one persistent launch (csrc/tp_layers.h: one workgroup per
 * CU, each op's weight share in registers before its input arrives, the edges as tagged granules, the residual
 * exchange per workgroup inside the launch), then the LM head launches. Taken for batch-1 fp16 models at head_dim
 * 128 whose per-workgroup shares fit (the TP-4 / TP-8 shards of Llama-2-7B); otherwise SLI_ERR_STATE with the
 * reason. Under tensor parallelism it needs the one-shot buffers and SLI_ALLREDUCE_FUSED_WG (ranks on distinct
 * devices), or no communicator (SLI_DEBUG_NOCOMM). Not for the ranks of an in-process group.
 * (Round 5 removed the opt-in persistent one-launch step, mode 1; sli_model_set_exec(1) returns SLI_ERR_ARG.) */
enum { SLI_EXEC_LAUNCHES = 0, SLI_EXEC_PERSIST = 2 };
int sli_model_set_exec(sli_model* m, int32_t mode);
int sli_model_get_exec(sli_model* m, int32_t* mode);
/* Sampling inside the step (the rule at sli_sample). p == NULL or p->temperature == 0: greedy, the default and the
 * reference's behaviour. Otherwise every step draws one token per sequence from its logits, as sequence b (the row
 * of the batch) at the position of the token just fed, between the LM head and the key reduce; past the prompt the
 * drawn token is what the state feeds next and what the history records. Prompt tokens stay teacher-forced, and
 * last_argmax goes on reporting the greedy argmax. The parameters live in device memory: changing them while
 * sampling is on re-captures nothing; turning sampling on or off drops the step graph (as sli_model_set_exec does),
 * and with sampling off the graph is the greedy one, node for node. Every weight and cache type, batch 1 .. 8, after
 * sli_model_prefill too. SLI_ERR_STATE with the reason for tp_size > 1 and for the ranks of an in-process group
 * (their logits are vocab-sharded) and under SLI_EXEC_PERSIST; sli_model_set_exec(SLI_EXEC_PERSIST) is refused the
 * same way while sampling is on. Parameters out of range are SLI_ERR_ARG before the device is touched.
 * sli_model_get_sampling: the parameters in force (temperature 0 while off).
 * sli_model_get_sampled: the token sequence `seq` drew in the last step; -1 while sampling is off or before a step.
 * sli_model_graph_captures: how many times the step graph has been captured since the model was created. */
int sli_model_set_sampling(sli_model* m, const sli_sampling* p);
int sli_model_get_sampling(sli_model* m, sli_sampling* out);
int sli_model_get_sampled(sli_model* m, int32_t seq, int32_t* token);
int sli_model_graph_captures(sli_model* m, int32_t* n);
/* Per-sequence generation inside the step (the rule at sli_sample_gen). sli_model_set_gen_seq gives sequence `seq` a
 * block of its own; p == NULL returns it to the default: greedy, no penalties, no stop. The first call puts the model
 * into per-sequence mode, which drops the step graph as turning sampling on does; from then on a change of any block
 * re-captures nothing (the table lives in device memory). The per-sequence step is: LM head, the per-row sampler over
 * the model's own history (csrc/gen_sample.h), key reduce, the sampled state update, then the stop launch.
 * last_argmax stays the greedy argmax of the raw logits, sli_model_get_logits stays raw, sli_model_get_sampled
 * reports the row's token. Any call of sli_model_set_sampling (NULL included) leaves the mode: it clears every block
 * and restores that call's behaviour and graphs, node for node.
 * The stop rule runs after the state update, one thread per sequence, and looks only at a sequence that is advancing
 * and has just moved to a position p >= n_forced (its token at p was chosen, not forced): that token in stop[0 ..
 * n_stop) gives SLI_FIN_STOP; else (max_pos > 0 and p >= max_pos) or p == max_len - 1 gives SLI_FIN_LENGTH. A finished
 * sequence gets advance = 0: it is parked at (token, p), the token stays in the history, and its later steps are
 * idempotent. A waiting sequence is never examined. A host call that writes a sequence's state clears its flag:
 * sli_model_set_state(_seq), the prefill / extend / score routes, sli_model_copy_prefix's destination,
 * sli_model_reset, and sli_model_set_gen_seq for that sequence.
 * Beyond sli_sample_gen's ranges (SLI_ERR_ARG), SLI_ERR_RANGE before anything is written for seq outside [0, batch),
 * a stop[i] outside [0, vocab) or max_pos > max_len - 1; SLI_ERR_SHAPE for a block with an active penalty on a model
 * beyond the penalised sampler's capacity (vocab > 262144 or max_len > 4096: such a model takes every other block,
 * stop conditions included); SLI_ERR_STATE with the reason as sli_model_set_sampling refuses: tp_size > 1,
 * the ranks of an in-process group, SLI_EXEC_PERSIST (in either order of the setters). Every weight and cache type,
 * batch 1 .. 8, after every prefill route.
 * sli_model_get_gen_seq: the block in force (the default block outside the mode). sli_model_get_finished: out[b] = 0,
 * SLI_FIN_STOP or SLI_FIN_LENGTH for every sequence of the batch (all 0 outside the mode). */
enum { SLI_FIN_STOP = 1, SLI_FIN_LENGTH = 2 };
int sli_model_set_gen_seq(sli_model* m, int32_t seq, const sli_gen_params* p);
int sli_model_get_gen_seq(sli_model* m, int32_t seq, sli_gen_params* out);
int sli_model_get_finished(sli_model* m, int32_t* out /* [batch] */);
/* One decode step (hipGraph replay; captured on first use). Asynchronous on the model's stream. */
int sli_model_step(sli_model* m);
/* Host waits (sync, logits / state / history reads, predict, prefill, the timing probes) of a rank whose step
 * carries RCCL collectives are bounded (csrc/comm_wait.h): they poll the stream, ncclCommGetAsyncError and a
 * deadline; a communicator error returns SLI_ERR_COMM, an expired deadline SLI_ERR_TIMEOUT, and either aborts the
 * communicator (ncclCommAbort), after which every call that would step returns SLI_ERR_COMM. The reference's
 * all-reduce-free equivalents: the logits copy at model.cpp:175-179. */
int sli_model_sync(sli_model* m);
/* logits of the last step: this rank's vocab shard [vocab_lo, vocab_lo+n) of every sequence, [batch][n]. */
int sli_model_get_logits(sli_model* m, float* host, int32_t n, int32_t* vocab_lo);
/* LlamaModel::predict on token ids: tokens_out[t] = token fed at position t; logits_out optional
 * [max_length][local vocab]. batch > 1: every sequence gets the prompt, tokens_out is [batch][max_length]
 * and logits_out [max_length][batch][local vocab]. */
int sli_model_predict(sli_model* m, const int32_t* prompt, int32_t n_prompt, int32_t max_length,
                      int32_t* tokens_out, float* logits_out);
/* predict for batch sequences with their own prompts: prompts [batch][ld] (sequence b's first lens[b]
 * ids), tokens_out [batch][max_length], logits_out optional [max_length][batch][local vocab]. */
int sli_model_predict_batch(sli_model* m, const int32_t* prompts, const int32_t* lens, int32_t ld, int32_t max_length,
                            int32_t* tokens_out, float* logits_out);
/* Copy one layer's K (which=0) or V (which=1) cache, positions [0, upto), to host as fp32 in reference
 * layout [upto][KV_local]. */
int sli_model_get_kv(sli_model* m, int32_t layer, int32_t which, int32_t upto, float* host);
int sli_model_get_kv_seq(sli_model* m, int32_t seq, int32_t layer, int32_t which, int32_t upto, float* host);
/* Read back this rank's shard of a weight (sli_tp_plan window, n = n_rows * n_cols) as fp32 (int8 is
 * dequantised with its row scales, MXFP4 with its block scales). */
int sli_model_get_weight(sli_model* m, int32_t kind, int32_t index, float* host, int64_t n);
int sli_model_stream(sli_model* m, sli_stream_t* out);
/* Algorithmic HBM bytes of one step on this rank (weights, KV at the current position) — SURVEY.md §8(d). */
int sli_model_step_bytes(sli_model* m, double* weight_bytes, double* kv_bytes);
/* ---------------------------------------------------------------- in-process tensor parallelism
 * The SURVEY.md §4 item-5 "fake communicator" (the reference drives one device, model.cpp:247-256):
 * tp_size rank models of cfg (cfg->tp_rank is ignored; rank r gets the sli_tp_plan shard of rank r)
 * on cfg->device, sharing one stream and stepped in lockstep by one captured hipGraph. Every all-reduce
 * of the multi-GPU step (the residual-stream sum after wo and down, the argmax-key MAX after the LM
 * head) is a device-side reduction over the ranks' buffers in rank order; the ranks' kernels are the
 * multi-GPU ones. Rank handles (sli_tp_group_rank) are borrowed: load weights, set state / prompts and
 * read logits through them; step and destroy only through the group. */
typedef struct sli_tp_group sli_tp_group;
int sli_tp_group_create(const sli_model_config* cfg, int32_t tp_size, sli_tp_group** out);
/* The same with the creation flags of sli_model_create_flags, applied to every rank; flags = 0 is sli_tp_group_create. */
int sli_tp_group_create_flags(const sli_model_config* cfg, int32_t tp_size, uint32_t flags, sli_tp_group** out);
int sli_tp_group_destroy(sli_tp_group* g);
int sli_tp_group_rank(sli_tp_group* g, int32_t rank, sli_model** out);
int sli_tp_group_step(sli_tp_group* g);
int sli_tp_group_sync(sli_tp_group* g);
/* sli_model_predict_batch over the group: tokens_out [batch][max_length]; logits_out optional
 * [max_length][batch][vocab] with the ranks' vocab shards in place (the full vocabulary). */
int sli_tp_group_predict_batch(sli_tp_group* g, const int32_t* prompts, const int32_t* lens, int32_t ld,
                               int32_t max_length, int32_t* tokens_out, float* logits_out);
/* sli_model_prefill / sli_model_predict_prefill over the group (batch-1 groups): the ranks' prefill chunks
 * run in lockstep, the residual rows summed over the ranks after every wo and down GEMM. logits_out
 * [max_length][vocab] (rows < n_prompt - 1 NaN). */
int sli_tp_group_prefill(sli_tp_group* g, const int32_t* ids, int32_t n);
int sli_tp_group_predict_prefill(sli_tp_group* g, const int32_t* prompt, int32_t n_prompt, int32_t max_length,
                                 int32_t* tokens_out, float* logits_out);
/* sli_model_set_prefill for every rank of the group. */
int sli_tp_group_set_prefill(sli_tp_group* g, int32_t mode);
/* sli_model_extend over the group (batch-1 groups): every rank continues from the start in lockstep, on the GEMM
 * chunks or teacher-forced through the group's decode step as sli_tp_group_prefill chooses. */
int sli_tp_group_extend(sli_tp_group* g, const int32_t* tokens, int32_t start, int32_t count);
/* sli_model_copy_prefix on every rank's shard of the cache. */
int sli_tp_group_copy_prefix(sli_tp_group* g, int32_t src, int32_t dst, int32_t n);

/* Roofline probe: replays the step's weight-streaming (GEMV) kernels `iters` times between HIP events
 * on the model's stream; returns mean device time per GEMV launch, algorithmic bytes per launch and
 * the launches per step. */
int sli_model_time_gemv(sli_model* m, int32_t iters, double* avg_us, double* bytes_per_launch,
                        int32_t* launches_per_step);
/* Device time of one replayed step: `iters` graph launches between HIP events on the model's stream. */
int sli_model_time_steps(sli_model* m, int32_t iters, double* avg_us);
/* Per-kernel-family probe: for each family f (sli_kernel_family) replays that family's launches of one
 * step `iters` times between HIP events on the model's stream; us[f] = mean device time per launch,
 * bytes[f] = algorithmic HBM bytes per launch (the weight matrix (+ int8 row scales),
 * or K and V of the live context for attention), launches[f] = launches per step. Arrays of
 * SLI_FAM_COUNT. */
typedef enum { SLI_FAM_QKV = 0, SLI_FAM_ATTN, SLI_FAM_WO, SLI_FAM_GU, SLI_FAM_DOWN, SLI_FAM_LM, SLI_FAM_COUNT } sli_kernel_family;
int sli_model_time_families(sli_model* m, int32_t iters, double* us, double* bytes, int32_t* launches);
/* The measured streaming-read floor of the same launches: for each family, a pure read kernel (no
 * arithmetic, 16-byte non-temporal loads, one 1024-thread workgroup per CU) over exactly the buffers that
 * family's launches stream (each layer's weight matrix; K and V of the layer for attention, the
 * allocated context), replayed the same way; us[f] = mean device µs per launch (the
 * fraction of a measured stream-copy bandwidth). */
int sli_model_time_stream(sli_model* m, int32_t iters, double* us);
/* Test hook (no device needed): runs the bounded-wait policy of comm_wait.h against mocked probes. mode 0: a
 * query that completes on its 3rd poll (SLI_OK); 1: a query that never completes (SLI_ERR_TIMEOUT after
 * deadline_ms); 2: an async communicator error on the 2nd poll (SLI_ERR_COMM); 3: a failing query (SLI_ERR_HIP).
 * *waited_ms = the wall time the wait took. */
int sli_debug_bounded_wait(int32_t mode, double deadline_ms, double* waited_ms);

/* ---------------------------------------------------------------- prefill stages, for tests and labs
 * The kernels of the prompt prefill (csrc/prefill.h), one launch each, without a model: device pointers and a
 * stream, as sli_matmul. The tiling of the GEMM and the attention kernel are chosen by the functions the engine's
 * prefill uses (prefill.h pg_pick, launch_pf_attn), so what runs here is what sli_model_prefill runs. fp16 arrays
 * ("hi" / "lo" operands, fp16 caches) are IEEE binary16. Every device pointer is 16-byte aligned. Anything the
 * kernels cannot take is SLI_ERR_ARG.
 * One row map: which prompt position a chunk row is stands in a device-resident group table (prefill.h PfSegs), 16 rows
 * to a group. `state` (the plain entries) and `table` (the *_segs entries) are SLI_PF_TABLE_BYTES of device memory that
 * the call fills on the stream ahead of the launch. The plain entries take (p0, nv) and write the table of one sequence
 * at consecutive positions: group g < M / 16 is {sequence 0, p0 + 16 g, clamp(nv - 16 g, 0, 16) valid rows}, any p0 >= 0;
 * `state` is 8-byte aligned. The *_segs entries take the groups themselves.
 *
 * sli_prefill_norm_split: x [M][D] fp32 -> hi, lo [M][D] fp16: h = RMSNorm(x row) * w (w NULL: h = x),
 * hi = fp16(h), lo = fp16(h - hi). D % 4 == 0, D <= 8192, M >= 1. */
#define SLI_PF_TABLE_BYTES 192 /* the group table: 3 int32 arrays (sequence, first position, valid rows) of 16 groups */
int sli_prefill_norm_split(const float* x, const float* w, void* hi, void* lo, int32_t M, int32_t D, float eps,
                           sli_stream_t stream);

/* The tiling a sli_prefill_gemm call ran (prefill.h PgCfg): a workgroup owns 16 * AT * WR weight rows x BM chunk
 * rows; S stages in the LDS ring, PIPE the pipelined fragment reads, SA > 0 the depth of the weights' own ring, KS
 * the depth (k) one stage covers. */
typedef struct {
    int32_t BM, WR, S, AT, PIPE, SA;
    int32_t KS;
} sli_pgemm_tiling;

/* The fused epilogue of a sli_prefill_gemm call; the fields of the other roles are ignored.
 * role 0, q/k/v: N = (hq + 2 hkv) * hd rows [q heads; k heads; v heads], hd 64 or 128. Row scale, then rotate-half
 *   RoPE of the q and k rows at position p0 + m (clamped to T - 1) with sin_t / cos_t [T][hd / 2]; q [M][hq * hd]
 *   fp32 is stored for every chunk row m < M; the K and V rows go to kc / vc, one layer's cache [hkv][T][hd] in
 *   kv_dtype (SLI_DT_F16 / SLI_DT_F32 / SLI_DT_F8E4M3: codes by the rule at sli_quant_f8, two per 2-byte store), at
 *   position p0 + m for m < nv and p0 + m < T only.
 * role 1, gate/up: N = 2 * inter rows [gate; up]; sigmoid(g) * u (act_mode 0) or SiLU(g) * u (1) as fp16 hi / lo
 *   in ahi / alo [M][inter].
 * role 2, wo / down: y[m][r] = (resid ? resid[m][r] : 0) + sum * row scale, y and resid [M][ld] fp32, ld >= N,
 *   ld % 4 == 0 (resid may be y).
 * role 3, logits (the LM head over chunk rows): y[m][r] = sum * row scale for r < N, through role 2's y / ld fields;
 *   no residual. N >= 16 need not be a multiple of 16 (the last tile's weight rows are clamped, the store and the row
 *   scale load masked at N); columns N .. ld - 1 of y are never written. ld >= N, ld % 4 == 0. For N % 16 == 0 the
 *   result is role 2's with a null resid, bit for bit. */
typedef struct {
    int32_t role;
    /* role 0 */
    float* q;
    void* kc;
    void* vc;
    int32_t kv_dtype;
    const float* sin_t;
    const float* cos_t;
    int32_t hq, hkv, hd, T;
    /* role 1 */
    void* ahi;
    void* alo;
    int32_t inter, act_mode;
    /* role 2 */
    float* y;
    const float* resid;
    int32_t ld;
} sli_pgemm_epilogue;

/* One pgemm_kernel launch: sums[m][r] = sum_k W[r][k] * (hi[m][k] + lo[m][k]) in fp32 on MFMA, then the epilogue.
 * W [N][K] in w_dtype (SLI_DT_F16 / SLI_DT_I8), w_row_scale [N] or NULL, hi / lo [M][K] fp16, M one of 32, 64,
 * 128, 256, K % 64 == 0, N % 16 == 0 (role 3: N >= 16), 0 <= p0, 1 <= nv <= M. *tiling (optional) receives the tiling that ran. */
int sli_prefill_gemm(const void* w, int w_dtype, const float* w_row_scale, const void* hi, const void* lo, int32_t N,
                     int32_t K, int32_t M, int32_t p0, int32_t nv, const sli_pgemm_epilogue* epi, void* state,
                     sli_pgemm_tiling* tiling, sli_stream_t stream);
/* sli_prefill_gemm for MXFP4 weights (beside it as sli_matmul_mxfp4 is beside sli_matmul): data uint8 [N][K / 2],
 * scales uint8 [N][K / 32] in the public layout (element 2i in bits 3:0 of byte i, scale 2^(byte - 127)); one
 * pgemm_kernel launch in its MXFP4 format, the code object an MXFP4 model's GEMM prefill launches. The same checks;
 * data is 16-byte aligned, scales need no alignment (they are loaded by the byte). The epilogues apply no row scale. Scale bytes
 * 1 .. 254 are exact (the block scale is applied in fp32). */
int sli_prefill_gemm_mxfp4(const void* data, const void* scales, const void* hi, const void* lo, int32_t N, int32_t K,
                           int32_t M, int32_t p0, int32_t nv, const sli_pgemm_epilogue* epi, void* state,
                           sli_pgemm_tiling* tiling, sli_stream_t stream);

/* Block-causal attention of M chunk rows (32, 64, 128 or 256): row m of head h attends the cache rows 0 .. p0 + m
 * of kv head h / (hq / hkv); q [rows][hq * hd] fp32, kc / vc one layer's cache [hkv][T][hd] in kv_dtype, the result
 * as fp16 hi / lo in ohi / olo [rows][hq * hd]. hd 64 or 128, hq % hkv == 0, 0 <= p0 < T. SLI_DT_F16 runs
 * and SLI_DT_F8E4M3 run pf_attn_mfma_kernel (one body, the cache format a template argument), SLI_DT_F32
 * pf_attn_kernel; the bases q, kc, vc, ohi, olo are 16-byte aligned for every dtype. Rows at positions >= T are
 * computed from clamped cache reads and mean nothing.
 * Buffer contract: the fp32-cache kernel works in blocks of 64 chunk rows, so at M = 32 it reads q and writes
 * ohi / olo for rows 32 .. 63 as well. rows_allocated is the number of rows q, ohi and olo really hold; the call is
 * refused unless it covers the rows the kernel touches (M for an fp16 or FP8 cache, M rounded up to 64 for fp32). */
int sli_prefill_attn(const float* q, const void* kc, const void* vc, int kv_dtype, void* ohi, void* olo, int32_t M,
                     int32_t rows_allocated, int32_t p0, int32_t hq, int32_t hkv, int32_t hd, int32_t T, void* state,
                     sli_stream_t stream);

/* The same two stages under a group table (sli_model_prefill_seqs): groups is a host array of M / 16 entries, chunk
 * rows 16 g .. 16 g + 15 being positions p0 .. p0 + 15 of sequence seq (p0 % 16 == 0, 0 <= p0 < T, 0 <= seq < B,
 * 0 <= nv <= 16; nv == 0: a padding group); `table` is SLI_PF_TABLE_BYTES of device memory (4-byte aligned) that the call
 * fills on the stream ahead of the launch. kc / vc are one layer's cache of all B sequences,
 * [B][hkv][T][hd], in SLI_DT_F16 or SLI_DT_F8E4M3 (an fp32 cache has no table form: SLI_ERR_ARG). The same pickers, so
 * what runs here is what sli_model_prefill_seqs runs.
 * sli_prefill_gemm_qkv_segs: the q/k/v GEMM (epi->role 0) with the table epilogue: q [M][hq * hd] gets every chunk
 *   row, RoPE at p0 + r (clamped to T - 1); the K / V rows of group g go to sequence seq's cache at p0 + r for
 *   r < nv and p0 + r < T only. _mxfp4: the MXFP4 twin (sli_prefill_gemm_mxfp4).
 * sli_prefill_attn_segs: group g's 16 rows attend sequence seq's cache rows 0 .. p0 + r; the rows of a padding group
 *   are left as they were. */
int sli_prefill_gemm_qkv_segs(const void* w, int w_dtype, const float* w_row_scale, const void* hi, const void* lo,
                              int32_t N, int32_t K, int32_t M, const sli_pf_group* groups, int32_t B,
                              const sli_pgemm_epilogue* epi, void* table, sli_pgemm_tiling* tiling, sli_stream_t stream);
int sli_prefill_gemm_qkv_segs_mxfp4(const void* data, const void* scales, const void* hi, const void* lo, int32_t N,
                                    int32_t K, int32_t M, const sli_pf_group* groups, int32_t B,
                                    const sli_pgemm_epilogue* epi, void* table, sli_pgemm_tiling* tiling,
                                    sli_stream_t stream);
int sli_prefill_attn_segs(const float* q, const void* kc, const void* vc, int kv_dtype, void* ohi, void* olo, int32_t M,
                          const sli_pf_group* groups, int32_t B, int32_t hq, int32_t hkv, int32_t hd, int32_t T,
                          void* table, sli_stream_t stream);

/* ---------------------------------------------------------------- batched decode stages, for tests and labs
 * One projection launch of the batched decode step (csrc/bgemm.h bgemm_kernel, 2 .. 8 sequences in lockstep; B = 1
 * is taken too), without a model: device pointers and a stream. The entry is compiled into the engine's translation
 * unit over the engine's own template arguments, so it launches the very code objects a model step launches: every
 * (role, weight type, cache type, layout) here is one the engine runs, and nothing else can be asked for. Role and
 * RMSNorm are paired as the engine pairs them: q/k/v, gate/up and logits take norm_w, store refuses it.
 *
 * The launch: sums[b][r] = sum_k W[r][k] * h[b][k] on MFMA with fp32 accumulation, h = x (store) or x * norm_w, the
 * fp32 h carried as fp16 hi + lo. With a norm the per-sequence 1 / sqrt(mean(x^2) + eps) multiplies the finished sum
 * (it commutes with the k-sum); then the row scale (w_row_scale[r], NULL: none), then the epilogue:
 * SLI_BG_QKV      rows [q heads; k heads; v heads] of hd (64 or 128) each, hq % hkv == 0, (hq + 2 hkv) hd % 16 == 0.
 *                 Rotate-half RoPE of the q and k rows at sequence b's position pos[b] with sin_t / cos_t
 *                 [T][hd / 2]; q [B][hq hd] fp32; the k and v rows go to kc / vc, one layer's cache [B][hkv][T][hd]
 *                 in kv_dtype (SLI_DT_F32 / F16 / F8E4M3), at row pos[b] of sequence b. pos is int32 [B] ON THE
 *                 DEVICE; 0 <= pos[b] < T is the caller's contract (the host cannot check it).
 * SLI_BG_GATE_UP  rows [gate (inter); up (inter)], inter % 8 == 0: act [B][inter] fp32 = sigmoid(g) * u (act_mode
 *                 0) or SiLU(g) * u (1).
 * SLI_BG_STORE    y[b][r] = (resid ? resid[b][r] : 0) + sum * scale for r < nrows; y and resid [B][ld] fp32,
 *                 ld >= nrows; resid may be y (the engine's residual stream is updated in place).
 * SLI_BG_LOGITS   logits[b][r] = sum for r < nrows, [B][ld]; keys_out [B][key_ld] uint64 receives, per sequence
 *                 and workgroup group g < plan.groups, the largest key of the group's rows: (orderable image of
 *                 the fp32 logit) << 32 | (0xFFFFFFFF - (vocab_off + r)), so the maximum over the groups names
 *                 the largest logit and, among equals, the lowest row (-0 counts as +0). key_ld >= groups.
 * Columns [nrows, ld) of y / logits, entries [groups, key_ld) of keys_out and every cache row but pos[b] are not
 * written. The fields of the other roles are ignored. */
enum { SLI_BG_QKV = 0, SLI_BG_GATE_UP = 1, SLI_BG_STORE = 2, SLI_BG_LOGITS = 3 };
typedef struct {
    int32_t role;
    /* SLI_BG_QKV */
    float* q;
    void* kc;
    void* vc;
    int32_t kv_dtype;
    const int32_t* pos;
    const float* sin_t;
    const float* cos_t;
    int32_t hq, hkv, hd, T;
    /* SLI_BG_GATE_UP */
    float* act;
    int32_t inter, act_mode;
    /* SLI_BG_STORE */
    float* y;
    const float* resid;
    float scale;
    /* SLI_BG_STORE and SLI_BG_LOGITS */
    int32_t nrows, ld;
    /* SLI_BG_LOGITS */
    float* logits;
    uint64_t* keys_out;
    int32_t vocab_off, key_ld;
} sli_bgemm_epilogue;

/* The plan of a launch, in / out. A workgroup owns tpw consecutive 16-row tiles and one of `splits` k-ranges;
 * groups = ceil(tiles / tpw) and the grid is groups * splits workgroups. On entry tpw == 0 asks the engine's planner
 * (bgemm.h bg_plan with the device's CU count: what a model of this shape runs); tpw != 0 forces (tpw, splits). A
 * forced plan must satisfy what the kernel assumes, or the call is SLI_ERR_ARG and nothing is launched: tpw >= 1,
 * splits >= 1; splits == 1 with a norm; splits > 1 only while (K / 32) / splits >= 16; ceil(K / 32 / splits) * 32 <=
 * 4096 (the staging registers); the LDS image 1 KiB + ceil(K / 32 / splits) KiB + 16 KiB + tpw / 2 KiB within 160 KiB.
 * On return every field holds what ran: step_width is the number of k-blocks a wave loads per step (2, 4 or 7: the
 * kernel instantiation), lds_bytes the dynamic LDS, counter_off the byte offset of the groups' arrival counters
 * (uint32 [groups]) inside the workspace. */
typedef struct {
    int32_t tpw, splits, groups, step_width, lds_bytes;
    int64_t counter_off;
} sli_bgemm_plan;

/* Bytes of workspace a sli_batch_gemm call needs for a [rows][K] matrix (rows: (hq + 2 hkv) hd, 2 inter or nrows),
 * and *plan resolved as the call would resolve it (no device needed): the split partials and arrival counters, plus
 * for tiled != 0 the fragment-layout image of W. 0 when the shape or the forced plan is refused. */
size_t sli_batch_gemm_workspace_bytes(int32_t rows, int32_t K, int32_t B, int32_t norm, int32_t w_dtype, int32_t tiled,
                                      sli_bgemm_plan* plan);

/* One bgemm_kernel launch. x [B][K] fp32, norm_w [K] fp32 or NULL (see the roles), W [rows][K] row-major in w_dtype
 * (SLI_DT_F16 / SLI_DT_I8), K % 32 == 0, 1 <= B <= 8. tiled != 0: the call first re-lays W into the fragment layout
 * inside the workspace with bg_tile_kernel and the epilogue's row map (RoPE pairs, gate/up pairs, the clamped last
 * tile), as a model does when weights are placed, and streams that image. Every device pointer is 16-byte aligned.
 * The arrival counters must be zero before the first call on a workspace (zero it once); a launch leaves them zero,
 * so later calls with the same plan reuse the workspace as it is. Anything the kernel cannot take is SLI_ERR_ARG,
 * decided before the device is touched. */
int sli_batch_gemm(const float* x, const float* norm_w, float eps, const void* w, int w_dtype, const float* w_row_scale,
                   int32_t tiled, int32_t K, int32_t B, const sli_bgemm_epilogue* epi, sli_bgemm_plan* plan,
                   void* workspace, size_t workspace_bytes, sli_stream_t stream);

/* sli_batch_gemm from MXFP4 weights: `data` uint8 [rows][K / 2] and `scales` uint8 [rows][K / 32] in the public
 * layout (sli_quant_mxfp4). The contract is sli_batch_gemm's word for word: the roles and their norm pairing, forced
 * plans and the refusals of plans the kernel cannot take, *plan filled with what ran, the counters left zero,
 * everything refused as SLI_ERR_ARG before the device is touched. There is no row scale: each 32-column block's
 * MFMA tile is multiplied by its block scale in fp32 before it joins the row sum. tiled != 0: the call first builds
 * the fragment-layout data image and the scale image (16 bytes per tile and k-block: the scales of the tile's rows in
 * the epilogue's row order) inside the workspace and streams those, as a batched MXFP4 model does. */
size_t sli_batch_gemm_mxfp4_workspace_bytes(int32_t rows, int32_t K, int32_t B, int32_t norm, int32_t tiled,
                                            sli_bgemm_plan* plan);
int sli_batch_gemm_mxfp4(const float* x, const float* norm_w, float eps, const void* data, const void* scales,
                         int32_t tiled, int32_t K, int32_t B, const sli_bgemm_epilogue* epi, sli_bgemm_plan* plan,
                         void* workspace, size_t workspace_bytes, sli_stream_t stream);

/* ---------------------------------------------------------------- decode stages, for tests and labs
 * One GEMV launch of the batch-1 decode step (csrc/gemv.h), without a model or a workspace (the GEMVs keep no
 * counters): device pointers and a stream. The entry is compiled into the engine's translation unit over the engine's
 * own template arguments, so it launches the very code objects a model step launches; role, input staging and RMSNorm
 * are paired as the engine pairs them, and nothing else can be asked for.
 *
 * The launch: the input vector h [cols] is staged once per workgroup as fp32, then sum[r] = sum_k W[r][k] h[k] with
 * fp32 accumulation, times the row scale (w_row_scale[r], NULL: none; MXFP4 has block scales instead), then the
 * epilogue. With a norm, h[k] = fl(fl(x[k] * inv) * norm_w[k]), inv = 1 / sqrtf(sum(x^2) / cols + eps).
 * SLI_GV_QKV      norm required. Rows [q heads; k heads; v heads] of hd (64 or 128) each, hq % hkv == 0. Rotate-half
 *                 RoPE of the q and k rows at *pos with sin_t / cos_t [T][hd / 2]; q [hq hd] fp32; the k and v rows go
 *                 to row *pos of kc / vc, one layer's cache [hkv][T][hd] in kv_dtype (SLI_DT_F32 / F16 / F8E4M3; not
 *                 F8E4M3 with fp32 weights). pos is int32 ON THE DEVICE; 0 <= *pos < T is the caller's contract.
 * SLI_GV_GATE_UP  norm required. Rows [gate (inter); up (inter)]: act [inter] fp32 = sigmoid(g) * u (act_mode 0) or
 *                 SiLU(g) * u (1). np = 2 or 4: the staged input is x + parts[0] + ... + parts[np - 1] (parts [np][cols],
 *                 added in that order, then normalised; cols <= 4096), the K-split wo's consumer.
 * SLI_GV_WO       no norm. y[r] = (resid ? resid[r] : 0) + sum for r < nrows; y may be resid (the residual stream is
 *                 updated in place) or not (a tensor-parallel rank). part == NULL: the input is x. part != NULL: the
 *                 input is merged from the attention's split partials part [hq][max_splits][hd + 4] (o[hd], m, l, pad)
 *                 while it is staged: over the ns = min(*pos / ppwg + 1, max_splits) live splits, in split order,
 *                 h = (sum_s e^(m_s - M) o_s) / (sum_s e^(m_s - M) l_s), M = max m_s; cols == hq * hd; max_splits > 8
 *                 takes the 16-split instantiation. ks = 2 or 4 (with part): the K-split wo, kpart[k][r] = the sum over
 *                 column block k of row r (times the row scale), no residual; hq % ks == 0.
 * SLI_GV_DOWN     no norm, input x. y[r] = (resid ? resid[r] : 0) + sum; np = 2 or 4: the residual is resid[r] +
 *                 parts[0][r] + ... + parts[np - 1][r] (parts [np][nrows]), in that order.
 * SLI_GV_LOGITS   norm required. logits[r] = sum for r < nrows; keys [key_ld] uint64 receives, per workgroup g <
 *                 plan.grid, the largest key of the rows it owned: (orderable image of the fp32 logit) << 32 |
 *                 (0xFFFFFFFF - (vocab_off + r)), 0 from a workgroup without rows. key_ld >= grid.
 * Nothing else is written. The fields of the other roles are ignored. */
enum { SLI_GV_QKV = 0, SLI_GV_GATE_UP = 1, SLI_GV_WO = 2, SLI_GV_DOWN = 3, SLI_GV_LOGITS = 4 };
typedef struct {
    int32_t role;
    /* SLI_GV_GATE_UP and SLI_GV_DOWN: the K-split wo's partial sums */
    const float* parts;
    int32_t np;
    /* SLI_GV_WO: the merged input and the K-split */
    const float* part;
    int32_t max_splits, ppwg, ks;
    float* kpart;
    /* SLI_GV_QKV (pos, hq, hd: SLI_GV_WO's merged input too) */
    const int32_t* pos;
    float* q;
    void* kc;
    void* vc;
    int32_t kv_dtype;
    const float* sin_t;
    const float* cos_t;
    int32_t hq, hkv, hd, T;
    /* SLI_GV_GATE_UP */
    float* act;
    int32_t inter, act_mode;
    /* SLI_GV_WO and SLI_GV_DOWN */
    float* y;
    const float* resid;
    /* SLI_GV_WO, SLI_GV_DOWN and SLI_GV_LOGITS */
    int32_t nrows;
    /* SLI_GV_LOGITS */
    float* logits;
    uint64_t* keys;
    int32_t vocab_off, key_ld;
} sli_gemv_epilogue;

/* The schedule of a launch, in / out. In: cus. 0: the device's compute units (what a model runs); otherwise the plan
 * is made by the engine's own planners as if the chip had `cus` compute units, 1 <= cus <= the device's, so a matrix
 * of a few hundred rows runs the schedule of a production one. Out, what ran: grid workgroups of 16 waves share
 * `units` units (R rows each) in balanced consecutive runs; a unit's row is cut into chunks_per_row chunks of u
 * 16-byte vectors per lane, masked_tail != 0 when the last chunk is partly past the row end; csplit column parts of
 * chunks_per_part chunks per unit (1: the whole row per wave); cw of the 16 waves stream; nb register buffers; ns the
 * split partials a thread holds in registers (merged input; 0 otherwise); lds_bytes the dynamic LDS. */
typedef struct {
    int32_t cus;
    int32_t grid, units, csplit, u, chunks_per_row, chunks_per_part, cw, nb, ns, masked_tail, lds_bytes;
} sli_gemv_plan;

/* *plan resolved as sli_decode_gemv (w_dtype SLI_DT_MXFP4: sli_decode_gemv_mxfp4) would resolve it, nothing launched;
 * only the shape fields of *epi are read, norm != 0 stands for norm_w. It needs no device when plan->cus != 0. */
int sli_decode_gemv_plan(int w_dtype, int32_t cols, int32_t norm, const sli_gemv_epilogue* epi, sli_gemv_plan* plan);

/* One launch. W [rows][cols] row-major in w_dtype (SLI_DT_F32 / F16 / I8), rows = (hq + 2 hkv) hd, 2 inter or nrows.
 * Refused as SLI_ERR_ARG, each with its own message, before the device is touched: a device pointer that is not
 * 16-byte aligned; cols not a multiple of the weight type's vector width (4, 8, 16; MXFP4 32) or above 16320; a role
 * and norm / staging pairing the engine does not make; hd other than 64 or 128, hq % hkv != 0; merged input with cols
 * != hq * hd; K-split with hq % ks != 0 or no grid that keeps every workgroup inside one column block; np > 0 at the
 * gate/up launch with cols > 4096; cus above the device's; more than 64 KiB of LDS; key_ld < grid. */
int sli_decode_gemv(const float* x, const float* norm_w, float eps, const void* w, int w_dtype, const float* w_row_scale,
                    int32_t cols, const sli_gemv_epilogue* epi, sli_gemv_plan* plan, sli_stream_t stream);

/* sli_decode_gemv from MXFP4 weights: `data` uint8 [rows][cols / 2] and `scales` uint8 [rows][cols / 32] in the public
 * layout (sli_quant_mxfp4); no row scale. The contract is sli_decode_gemv's. */
int sli_decode_gemv_mxfp4(const float* x, const float* norm_w, float eps, const void* data, const void* scales,
                          int32_t cols, const sli_gemv_epilogue* epi, sli_gemv_plan* plan, sli_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
