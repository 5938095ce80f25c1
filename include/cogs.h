/*
 * cogs.h -- C ABI of libcogs_hip.so: the MI355X (gfx950) hot path of the CogReasoner
 * streaming-VQA inference pipeline (reference: LiamZhao326/CogStream, model/ package).
 *
 * The reference has no native ABI: its hot path is Python calling torch / transformers /
 * flash-attn. This header is the boundary a maintainer binds with
 * ctypes from the three reference seams
 *     vision_encoder(pixel_values, grid_sizes, merge_sizes)   model/cogreasoner_chat.py:270-274
 *     kmeans_with_time_min_max(features, timestamps, K)        model/cogreasoner_chat.py:283
 *     get_model()(inputs_embeds=..) / super().generate(..)     model/cogreasoner_chat.py:312-316,802
 * (the stub is shown in INTEGRATION.md; cogstream_amd/_lib.py is the binding this repo uses).
 *
 * Rules that hold for every entry point:
 *   - extern "C", plain pointers and sizes; returns a cogs_status (0 = ok, negative = error);
 *     never throws, never synchronises the device unless stated, never allocates
 *     caller-visible memory (workspace sizes are queried, then passed in);
 *   - all tensor pointers are DEVICE pointers owned by the caller (e.g. torch tensors'
 *     data_ptr()); small shape arrays marked "host" are host pointers read during the call;
 *   - `stream` is a hipStream_t; work is enqueued on it in call order;
 *   - `dtype` is the storage + arithmetic input type of activations/weights:
 *     COGS_DT_BF16 (production; fp32 accumulation) or COGS_DT_F32 (parity mode, exact-f32 MFMA);
 *   - a handle is bound to one device; calls on one handle are not thread-safe. Calls may be queued on a stream
 *     back to back without synchronising: every device table a call needs is built by kernels on that stream or
 *     travels through a pinned, event-guarded staging ring of the handle, and the workspace passed to a call is
 *     only touched by work queued on the call's stream (so one workspace = one stream at a time).
 */
#ifndef COGS_H_
#define COGS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int cogs_status;
#define COGS_OK 0
#define COGS_E_INVALID (-1)     /* bad argument / unsupported shape alignment */
#define COGS_E_HIP (-2)         /* a HIP runtime call or kernel launch failed */
#define COGS_E_UNSUPPORTED (-3)
#define COGS_E_WORKSPACE (-4)   /* workspace missing or too small */

#define COGS_DT_BF16 0
#define COGS_DT_F32 1

#define COGS_ACT_NONE 0
#define COGS_ACT_GELU_TANH 1    /* ACT2FN["gelu_pytorch_tanh"], ViT fc1 */
#define COGS_ACT_GELU_ERF 2     /* nn.GELU(), projector */
#define COGS_ACT_SWIGLU 3       /* silu(gate)*up on (gate_i, up_i)-interleaved weight rows */

/* ViT attention semantics (SURVEY.md headline fact 2) */
#define COGS_ATTN_BLOCK_DIAG 0        /* per-frame attention = flash_attn_varlen path (:309-312) */
#define COGS_ATTN_REF_EAGER_GLOBAL 1  /* eager path: global attention, +1.0 logit on same-frame pairs (:257-266) */

typedef struct cogs_ctx* cogs_handle;
typedef void* cogs_stream; /* hipStream_t */

const char* cogs_status_string(cogs_status s);
const char* cogs_version(void);

cogs_status cogs_create(int device, cogs_handle* out);
cogs_status cogs_destroy(cogs_handle h);   /* NULL is accepted (no-op) */

/* Optional per-kernel-class timing of the composite calls below (HIP events on `stream`, recorded
 * around every launch between begin and end). Used by bench.py for the roofline figure; adds a few
 * microseconds per launch, so it is never on inside a throughput measurement. */
#define COGS_PROF_GEMM 0
#define COGS_PROF_ATTN 1
#define COGS_PROF_NORM 2
#define COGS_PROF_OTHER 3
#define COGS_PROF_CLASSES 4
cogs_status cogs_profile_begin(cogs_handle h);
/* synchronises `stream`; ms_per_class / launches_per_class: host arrays [COGS_PROF_CLASSES]; launches are KERNELS
 * (a GEMM that the library splits in two counts twice), so ms / launches is comparable with rocprofv3's kernel stats */
cogs_status cogs_profile_end(cogs_handle h, cogs_stream stream, float* ms_per_class, int* launches_per_class);

/* Diagnostics. The library reads NOTHING from the environment: its A/B switches (which kernel body a shape gets, timing-
 * only modes, prints) live in one table whose defaults are the shipped behaviour (cogstream_amd/csrc/debug.h lists them;
 * cogs_debug_list() returns the same text: "name = default: meaning" per line). bench.py --debug, tools/ and the
 * bit-identity tests flip a switch by name, run, and flip it back inside one process. Process-wide and unsynchronised:
 * set between calls. Unknown names return COGS_E_INVALID. cogs_debug_get also reports "gemm_last_body". */
cogs_status cogs_debug_set(const char* name, int64_t value);
cogs_status cogs_debug_get(const char* name, int64_t* value);
const char* cogs_debug_list(void);

/* ------------------------------------------------------------------ operator level ---- */

/* DESCRIPTORS (cogs_gemm_desc, cogs_attn_desc, ...) MUST BE ZERO-INITIALISED before the caller fills in what it uses
 * (`cogs_gemm_desc d = {0};` / memset / ctypes' default constructor): they carry no size or version member, new optional
 * fields are appended at the end with 0 = "off" (round 5: cogs_gemm_desc.hm_rows / hm_cols, cogs_attn_desc.head_stride), and a
 * field left holding stack garbage switches a feature on. cogs_version() names the ABI revision: "0.2" added those three,
 * "0.3" cogs_lm_score / cogs_row_lse, "0.4" cogs_gemv_fp8 / cogs_quantize_fp8_rows / cogs_llm_attach_fp8 (new entry points
 * only; every older signature and structure is unchanged). Added since without a new revision string (new entry points
 * and structures only): cogs_gemm_rows, cogs_attention_rows / cogs_attn_rows_desc, cogs_llm_decode_rows /
 * cogs_llm_decode_rows_workspace_bytes / cogs_kv_rows; cogs_attn_rows_desc.tail_slot / tail_slot_ld (appended, 0 = off),
 * cogs_llm_decode_rows_slots, cogs_beam_topk / cogs_beam_topk_workspace_bytes, cogs_sub_rows, cogs_gemm_rows_fp8,
 * cogs_gemm_fused / cogs_gemm_fused_args. */

/* C[M,N] = epilogue(A[M,K] . W[N,K]^T). nn.Linear / Conv2d(k=s=14) replacement
 * (model/modeling_videollama3_encoder.py:194-210,246-248,275,369-373; cogreasoner_chat.py:179-211).
 * K must be a multiple of 64 (bf16) / 32 (f32) -- pad with zeros; N a multiple of 4;
 * lda/ldw/ldc/ldr in elements. A and W rows must be 16-byte aligned (lda / ldw a multiple of 8 bf16 or 4 fp32 elements,
 * else COGS_E_INVALID). C and residual rows need only the alignment of four elements (ldc / ldr and the C / residual
 * pointers a multiple of 4 elements: 8 bytes for bf16); rows that are 16-byte aligned take the wide stores, others the
 * per-wave epilogue, with the same results. residual may alias C (ldr == ldc: in-place x += f(x)).
 * bias [N] and residual [M,N] nullable.
 * rope: if rope_cos != NULL, columns [0, rope_cols) are rotated with tables [M, head_dim/2] (fp32), or --
 * rope_sin == NULL -- with ONE interleaved table [M, head_dim/2, 2] = (cos, sin) in rope_cos (faster);
 * weight rows must be packed so that columns (2i, 2i+1) of a head are the rotate_half pair
 * (i, i + head_dim/2). act = COGS_ACT_*; SWIGLU writes [M, N/2]. out_f32: store fp32. */
typedef struct {
    int dtype;
    const void* A; int64_t lda;
    const void* W; int64_t ldw;
    void* C; int64_t ldc;
    const void* bias;
    const void* residual; int64_t ldr;
    int M, N, K;
    int act;
    int out_f32;
    const float* rope_cos;
    const float* rope_sin;
    int rope_cols;
    int head_dim;
    /* optional 2-D rotary position LUT (ViT): rope_lut [rope_maxpos][head_dim/4][2] fp32 = (cos, sin)(pos * inv_freq[f]),
     * rope_rowpos [M] int32 = h | w << 16; the first half of a head's pairs rotates with h, the second with w. Large
     * bf16 GEMMs then read the factors from an LDS copy of the LUT; rope_cos must still hold the matching interleaved
     * per-row table (rope_sin NULL) for the tiles that do not take that path. */
    const float* rope_lut;
    const int32_t* rope_rowpos;
    int rope_maxpos;
    /* LayerNorm fused around the GEMM (nn.LayerNorm of modeling_videollama3_encoder.py:382-391; bf16/f32 alike):
     * row_stats != NULL: the GEMM also writes, per output row and 64-column block, (sum, sum of squares) of the values
     *   it stores (after the rounding to `dtype`): row_stats [M][N/64][2] fp32 (N % 64 == 0, no SWIGLU / fp32 output); cogs_ln_finalize turns them into
     *   ln_ab [M][2] = (rstd, -rstd * mean).
     * ln_ab != NULL: the GEMM computes LN(A) . W0^T + bias0 WITHOUT a normalised copy of A. What the kernels evaluate
     *   is exactly  y[r][n] = ln_ab[r][0] * acc[r][n] + col_c[n]  (before rope / activation; bias must be NULL), where
     *   acc = A . W^T on the UN-normalised rows of A. That equals LN(A) . W0^T + bias0 if and only if the caller passes
     *     W [n][k]  = W0[n][k] * gamma[k] - mean_k(W0[n][:] * gamma)      (every row of W sums to ZERO over k: the
     *                 mean term  -rstd * mean_r * sum_k W[n][k]  of the LayerNorm then vanishes and is NOT evaluated;
     *                 ln_ab[r][1] is not read), stored in `dtype`;
     *     col_c [n] = bias0[n] + sum_k W0[n][k] * beta[k]                 (fp32 [N]).
     *   A W whose rows do not sum to zero gives wrong results without any error. The rounding of W to bf16 leaves a
     *   row sum s_n != 0, i.e. an error rstd * mean * s_n that grows with |mean / std| of a row of A;
     *   cogstream_amd.weights.fold_layernorm removes it by moving a handful of weights per row one bf16 step so that
     *   the ROUNDED row sums to zero too (|s_n| < one step of the row's smallest weights). The specialised
     *   epilogues that exist, all with M >= 2 and bf16 or fp32 inputs:
     *     row_stats: bias, bias + residual (the out-proj / fc2 form, residual in place included);
     *     ln_ab:     alone, + rope, + GELU_TANH, + rope + head-major output.
     *   Anything else together with ln_ab or row_stats returns COGS_E_UNSUPPORTED: M == 1, row_stats without bias, any
     *   activation with row_stats, residual / GELU_ERF / SWIGLU / fp32 output with ln_ab, fp32 output with row_stats.
     *   ln_ab with bias, ln_ab without col_c and row_stats with N % 64 != 0 return COGS_E_INVALID. */
    float* row_stats;
    const float* ln_ab;
    const float* col_c;
    /* Head-major output (bf16, M >= 2, no activation / residual / row_stats / fp32 output; what the encoder's QKV GEMM uses):
     * hm_rows > 0 -> the N columns are N / hm_cols blocks (q | k | v) of hm_cols / head_dim heads each, and element (row m,
     * column n) is stored at  C[((n / hm_cols) * (hm_cols / head_dim) + (n % hm_cols) / head_dim) * hm_rows * head_dim
     * + m * head_dim + n % head_dim]  -- [block][head][row][head_dim], every head's rows contiguous (ldc is ignored; M <=
     * hm_rows; head_dim % 8 == 0; hm_cols % head_dim == 0; N % hm_cols == 0; hm_rows * hm_cols * 2 < 2^32).
     * cogs_attn_desc.head_stride reads that layout. 0 = row-major C[m][n]. M == 1 or fp32 inputs return COGS_E_UNSUPPORTED,
     * an activation, a residual, fp32 output or a violated shape condition COGS_E_INVALID (row_stats: see above). */
    int64_t hm_rows;
    int hm_cols;
} cogs_gemm_desc;
cogs_status cogs_gemm(cogs_stream stream, const cogs_gemm_desc* d);
/* (rstd, -rstd * mean) per row from the row_stats partials of a GEMM whose N is the LayerNorm width H */
cogs_status cogs_ln_finalize(cogs_stream stream, const float* row_stats, int rows, int H, float eps, float* ln_ab);

/* C[M,N] = epilogue(A[M,K] . W[N,K]^T) for 1 <= M <= 16 rows in bf16: the GEMM of a lockstep decode step over several
 * sequences (cogs_llm_decode_rows). W is streamed exactly once, as the operand of v_mfma_f32_16x16x32_bf16 whose 16 columns
 * are the M rows (fp32 sums); a small N splits K over the waves of a workgroup and adds the parts in a fixed order -- no
 * floating-point atomics, the same call gives the same bits, and for a fixed M output row m holds the same bits whatever
 * the other rows hold and whichever slot it sits in. Takes cogs_gemm's descriptor and its shape rules: K % 64 == 0, N % 4 == 0,
 * lda / ldw multiples of 8 and >= K, A and W 16-byte aligned, ldc / ldr and the C / residual pointers multiples of 4 elements
 * (else COGS_E_INVALID). Epilogues: bias, rotary with per-row tables (interleaved when rope_sin == NULL), q_scale (0 or 1 = off)
 * on columns < q_cols (rotary epilogues only, as in cogs_gemv_fp8_desc), COGS_ACT_SWIGLU, residual (may alias C), out_f32.
 * COGS_E_UNSUPPORTED, before any launch: dtype != COGS_DT_BF16, M > 16, ln_ab, row_stats, hm_rows, rope_lut, the GELUs.
 * cogs_gemm does not dispatch here: its results for 2 <= M <= 16 stay what they were. */
cogs_status cogs_gemm_rows(cogs_stream stream, const cogs_gemm_desc* d, float q_scale, int q_cols);
/* cogs_gemm_rows on e4m3 weights: C[M,N] = epilogue(scale[n] * sum_k A[m,k] * e4m3(W[n][k])). d->W holds OCP e4m3fn codes
 * [N][ldw] (one byte per weight, ldw in BYTES; 0x7F / 0xFF must not occur), scale one fp32 POWER OF TWO per output column -- what
 * cogs_quantize_fp8_rows writes; every other field, the shape rules and the epilogues are cogs_gemm_rows's. The codes are the
 * streamed MFMA operand (half the bytes of the bf16 matrix), converted in registers; forms, k split and order of additions are
 * those of cogs_gemm_rows, and the scale multiplies the finished fp32 sum once. The result is therefore BIT-IDENTICAL to
 * cogs_gemm_rows on the dequantised matrix code * scale, wherever the dequantised weights are normal bf16 numbers and the
 * sums times scale normal fp32 numbers (a subnormal on either side is rounded on one side only).
 * COGS_E_INVALID: NULL scale, ldw % 16 != 0, ldw < K, W not 16-byte aligned, K % 64 != 0, N % 4 != 0 and what cogs_gemm_rows
 * rejects for A / C / residual. COGS_E_UNSUPPORTED, before any launch: what cogs_gemm_rows refuses (dtype != COGS_DT_BF16,
 * M > 16, ln_ab, row_stats, hm_rows, rope_lut, the GELUs). */
cogs_status cogs_gemm_rows_fp8(cogs_stream stream, const cogs_gemm_desc* d, const float* scale, float q_scale, int q_cols);

/* cogs_gemm with the fused pieces the Qwen2 layer adds around its linears (what cogs_llm_forward passes to the same
 * dispatcher): C[M,N] = epilogue(A[M,K] . W[N,K]^T) with cogs_gemm's descriptor, shape rules and choice of kernel, plus
 *   q_scale (0 or 1 = off): columns < q_cols are multiplied by it after bias / rotary, before the activation and the one
 *     rounding (any M; rotary epilogues only: rope_cos != NULL, q_cols % 4 == 0, q_cols <= rope_cols);
 *   rms_gamma != NULL (M == 1): A is replaced by Qwen2RMSNorm(A) = gamma * (A * rsqrt(mean(A^2) + rms_eps)) on the fly, with
 *     the roundings of cogs_rmsnorm (gamma [K] in `dtype`, 16-byte aligned);
 *   kv_k != NULL (M == 1): columns [kv_col0, kv_col0 + kv_dim) are written to kv_k[0..kv_dim) and the next kv_dim columns
 *     to kv_v[0..kv_dim) instead of C, in `dtype` (kv_col0 + 2 * kv_dim == N; those columns of C are not written).
 * M == 1 runs the weight-streaming GEMV (the bf16 / fp32 counterpart of cogs_gemv_fp8), M > 1 the planned body.
 * COGS_E_INVALID: a NULL d / args / A / W / C and what cogs_gemm rejects; q_scale without rope_cos, q_cols % 4 != 0 or q_cols >
 * rope_cols; with kv_k: a NULL kv_v, kv_col0 or kv_dim negative or not a multiple of 4, kv_col0 + 2 * kv_dim != N, out_f32,
 * COGS_ACT_SWIGLU. COGS_E_UNSUPPORTED, before any launch: rms_gamma or kv_k with M > 1 (the MFMA bodies know neither), and
 * what cogs_gemm refuses. A zero-initialised cogs_gemm_fused_args makes the call cogs_gemm. */
typedef struct {
    float q_scale; int q_cols;
    const void* rms_gamma; float rms_eps;
    void* kv_k; void* kv_v; int kv_col0; int kv_dim;
} cogs_gemm_fused_args;
cogs_status cogs_gemm_fused(cogs_stream stream, const cogs_gemm_desc* d, const cogs_gemm_fused_args* args);

/* W8A16 GEMV (single-token decode): C[N] = epilogue(scale[n] * sum_k x[k] * e4m3(W[n][k])). W holds OCP e4m3fn codes (one
 * byte per weight; 0x7F / 0xFF, the NaN codes, must not occur), scale one fp32 POWER OF TWO per output row -- what
 * cogs_quantize_fp8_rows writes -- so that a dequantised weight code * scale is exactly a bf16 value and the GEMV computes
 * what cogs_gemm computes on the dequantised matrix (other summation order). dtype (COGS_DT_*) is the type of x, bias,
 * residual, rms_gamma, C and the K / V row; sums are fp32. Epilogue as cogs_gemm with M = 1: bias, rotary (row tables
 * [head_dim/2], or one interleaved table when rope_sin == NULL) on columns < rope_cols, q_scale (0 or 1 = off) on columns <
 * q_cols, act, residual (may alias C), out_f32. rms_gamma != NULL: x is replaced by Qwen2RMSNorm(x) = gamma * (x *
 * rsqrt(mean(x^2) + rms_eps)) on the fly. kv_k != NULL: columns [kv_col0, kv_col0 + kv_dim) are written to kv_k[0..kv_dim)
 * and the next kv_dim columns to kv_v instead of C (kv_col0 + 2 * kv_dim == N; not with out_f32 / SWIGLU).
 * COGS_E_INVALID: a NULL x / W / scale / C, N % 4 != 0, K % 16 != 0, ldw % 16 != 0 or ldw < K, x / W / rms_gamma not 16-byte
 * aligned, a kv_col0 / kv_dim that is not a multiple of 4, and what cogs_gemm rejects for the same epilogue. */
typedef struct {
    int dtype;
    const void* x;                       /* [K] */
    const uint8_t* W; int64_t ldw;       /* [N][ldw] bytes */
    const float* scale;                  /* [N] */
    void* C;                             /* [N] (SWIGLU: [N/2]) */
    const void* bias;                    /* [N], nullable */
    const void* residual;                /* [N], nullable */
    int N, K;
    int act;
    int out_f32;
    const float* rope_cos;
    const float* rope_sin;
    int rope_cols;
    int head_dim;
    float q_scale; int q_cols;
    const void* rms_gamma; float rms_eps;
    void* kv_k; void* kv_v; int kv_col0; int kv_dim;
} cogs_gemv_fp8_desc;
cogs_status cogs_gemv_fp8(cogs_stream stream, const cogs_gemv_fp8_desc* d);

/* Row-wise e4m3 quantiser of the load path: w [N][ldw] (dtype bf16 / fp32, ldw in elements) -> codes [N][ldq] bytes and
 * scale [N] fp32 with scale[n] = 2^ceil(log2(absmax_n / 448)) (1 for an all-zero row, never below 2^-126), codes = w / scale
 * rounded to the nearest e4m3fn value, ties to even. dequant (nullable; may be w itself; ldd in elements): code * scale in
 * `dtype`, exact. Bit-equal to cogstream_amd.weights.quantize_fp8_rows, which is its specification. K % 16 == 0, rows of w /
 * dequant 16-byte aligned, ldq % 8 == 0, else COGS_E_INVALID. */
cogs_status cogs_quantize_fp8_rows(cogs_stream stream, int dtype, const void* w, int64_t ldw, int N, int K, uint8_t* codes,
                                   int64_t ldq, float* scale, void* dequant, int64_t ldd);

/* Attention over token-major Q/K/V (row stride ld*, head h at column h*head_dim).
 * cu_seqlens (device int32 [nseg+1], nullable): block-diagonal segments as in
 * flash_attn_varlen_func (modeling_videollama3_encoder.py:309-312, cu_seqlens :439-440).
 * row_lo/row_hi (device int32 [q_len], nullable): eager-reference mode, every query sees all
 * keys and `bias` is added to the logits of keys in [row_lo[q], row_hi[q]) (:257-266).
 * causal: key j visible to query i iff j <= i + q_pos0 (Qwen2; q_pos0 = kv_len - q_len).
 * nsplit > 1 splits the keys over workgroups (decode); ws >= nsplit*q_len*hq*(head_dim+2)*4 bytes (the library computes this
 * in one place: csrc/attn_plan.h, cogs_attn_split_ws_bytes; which kernel a descriptor gets: cogs_plan_attention there).
 * O: only rows [0, q_len) x columns [0, hq*head_dim) are written; the columns up to ldo and everything before and after
 * keep their bits. Keys past kv_len / past the last segment and Q rows past q_len are never given weight. */
typedef struct {
    int dtype;
    const void* Q; const void* K; const void* V; void* O;
    int64_t ldq, ldk, ldv, ldo;
    const int32_t* cu_seqlens; int nseg; int max_seqlen;
    const int32_t* row_lo; const int32_t* row_hi; float bias;
    int q_len, kv_len;
    int hq, hkv, head_dim;
    float scale;
    int causal; int q_pos0;
    int force_rowwise;      /* use the generic fp32-math kernel (any head_dim <= 256) */
    int nsplit; void* ws; size_t ws_bytes;
    int q_prescaled;        /* Q already carries scale*log2(e) (`scale` is then ignored): lets the bf16 kernels run the
                             * softmax without a per-score multiply; not with row_lo/row_hi */
    int64_t head_stride;    /* 0: token-major Q / K / V as described above (head h at column h*head_dim of a row). > 0: HEAD-major
                             * Q, K and V -- head h starts head_stride elements after head h-1 and holds its rows back to back
                             * (ldq = ldk = ldv = head_dim): the layout cogs_gemm_desc.hm_rows writes (head_stride = hm_rows *
                             * head_dim). Only the encoder's production shape takes it (bf16, head_dim 72, cu_seqlens, pre-scaled
                             * Q, hq == hkv, no mask modes); anything else returns COGS_E_UNSUPPORTED. O stays token-major. */
} cogs_attn_desc;
cogs_status cogs_attention(cogs_stream stream, const cogs_attn_desc* d);

/* Decode attention of `rows` (<= 16) sequences that share a prompt: query row r (hq heads, head_dim 128, bf16, already
 * multiplied by softmax_scale * log2(e)) sees keys [0, prefix_len) of the shared K / V (token-major, head h at column
 * h * 128, row strides ldk / ldv) and keys [0, tail_len) of its own tail at tail_k / tail_v + r * tail_row_stride (key
 * stride tail_ld; all strides in elements, multiples of 8). prefix_len >= 1, tail_len >= 1. Per kv head the rows * (hq / hkv)
 * query columns are packed into MFMA tiles of 16; the shared keys are split over nsplit (1 .. 127) workgroups per tile, every
 * row's tail is one more partial, and one combine kernel merges the nsplit + 1 partials. O: dense [rows][hq * 128].
 * ws >= (nsplit + 1) * rows * hq * (head_dim + 2) * 4 bytes (cogs_attn_split_ws_bytes with nsplit + 1 parts). COGS_E_UNSUPPORTED: dtype != COGS_DT_BF16, head_dim != 128,
 * hq / hkv > 16 or not integral, rows > 16. Zero-initialise the descriptor.
 * tail_slot (device int32, nullable): with a table, row r reads tail key j from tail_k / tail_v + tail_slot[r * tail_slot_ld + j] *
 * tail_row_stride + j * tail_ld instead of from its own slot r -- beam search, where a row continues the keys another row wrote
 * without copying them. Every entry the call reads (j < tail_len) must lie in [0, rows): the caller's contract, not checked on
 * the device (an entry outside is clamped into the range, so a bad table reads wrong keys, not foreign memory).
 * tail_slot_ld < tail_len returns COGS_E_INVALID. */
typedef struct {
    int dtype;
    const void* Q; int64_t ldq;
    const void* K; const void* V; int64_t ldk, ldv; int prefix_len;
    const void* tail_k; const void* tail_v; int64_t tail_ld, tail_row_stride; int tail_len;
    void* O;
    int rows, hq, hkv, head_dim;
    int nsplit; void* ws; size_t ws_bytes;
    const int32_t* tail_slot;
    int64_t tail_slot_ld;
} cogs_attn_rows_desc;
cogs_status cogs_attention_rows(cogs_stream stream, const cogs_attn_rows_desc* d);

/* nn.LayerNorm (modeling_videollama3_encoder.py:382-384,475) / Qwen2RMSNorm; H % 8 == 0 */
cogs_status cogs_layernorm(cogs_stream stream, int dtype, const void* x, void* y, const void* gamma,
                           const void* beta, int rows, int H, float eps);
cogs_status cogs_rmsnorm(cogs_stream stream, int dtype, const void* x, void* y, const void* gamma, int rows,
                         int H, float eps);
/* y[r] = mean_{i<group} LayerNorm(x[group*r+i]): post_layernorm + 2x2 bilinear merge (:482-501) */
cogs_status cogs_ln_merge(cogs_stream stream, int dtype, const void* x, void* y, const void* gamma,
                          const void* beta, int out_rows, int group, int H, float eps);

/* Pixel-difference keep-mask of merged visual tokens (model/cogreasoner_chat.py:405-422).
 * pix: one video's pixel_values viewed as [t, P, E] (E = merge^2 * 588); mask: uint8 [t*P].
 * minor (device uint8 [t], nullable): frames reduced to their token 0. */
cogs_status cogs_pixdiff_mask(cogs_stream stream, int dtype, const void* pix, int t, int P, int E, float thr,
                              int min_tokens, const uint8_t* minor, uint8_t* mask);
/* token 0 of each listed frame <- mean over the frame's P tokens, in place (cogreasoner_chat.py:434-447) */
cogs_status cogs_frame_mean_to_slot0(cogs_stream stream, int dtype, void* feats, int P, int D,
                                     const int32_t* frames, int n_frames);
/* out[r] = idx[r] >= 0 ? table_a[idx[r]] : table_b[-idx[r]-1]   (embed_tokens + masked scatter, :567-572) */
cogs_status cogs_gather_rows(cogs_stream stream, int dtype, const void* table_a, const void* table_b,
                             const int64_t* idx, void* out, int rows, int D);
/* out[D] (fp32) = mean over rows (torch.mean(last_hidden_state, dim=1), :317,323) */
cogs_status cogs_mean_rows(cogs_stream stream, int dtype, const void* x, int64_t ldx, int rows, int D, float* out);
/* out[i] = cos(a, b[i])  (F.cosine_similarity, :325) */
cogs_status cogs_cosine(cogs_stream stream, const float* a, const float* b, int n, int D, float* out);

/* Time-aware k-means steps (model/kmeans_with_time.py:4-137); the host keeps the RNG draws.
 * feats [T, PD] (dtype), centres fp32 [K, PD], ts/centre_ts fp32. Any T and K (the reference has no limit: a
 * 600-frame session clusters into K = 40). Distances are direct sums of (x - c)^2, not torch.cdist's
 * |x|^2 + |c|^2 - 2 x.c: see DESIGN.md section 2 (near-tie study) for where the reference's own rounding decides. */
cogs_status cogs_kmeans_workspace_bytes(int T, int64_t PD, int K, size_t* bytes);
/* dist2[T,K] = squared L2 distance to the centres; centre_rows (device int32 [K], nullable)
 * selects feature rows as centres instead of `centres` (k-means++ init, :46-50) */
cogs_status cogs_kmeans_sqdist(cogs_stream stream, int dtype, const void* feats, int T, int64_t PD,
                               const float* centres, const int32_t* centre_rows, int K, float* dist2,
                               void* ws, size_t ws_bytes);
/* per-row min-max normalised feature + time distance, argmin (:76-104); counts int32 [K] */
cogs_status cogs_kmeans_assign(cogs_stream stream, const float* dist2, const float* ts, const float* centre_ts,
                               int T, int K, float alpha, int64_t* assign, int32_t* counts);
/* centres/centre_ts <- cluster means, empty cluster k <- row reseed_rows[k] (:107-120);
 * shift_out[0] = sum_k ||dc_k||_2 + ||d centre_ts||_2 (:123-125) */
cogs_status cogs_kmeans_update(cogs_stream stream, int dtype, const void* feats, const float* ts, int T,
                               int64_t PD, int K, const int64_t* assign, const int32_t* reseed_rows,
                               float* centres, float* centre_ts, float* shift_out, void* ws, size_t ws_bytes);
/* select_additional_frames (model/cogreasoner_chat.py:50-64): per cluster k, the rows the event selection always keeps --
 * all members if there are at most n_extra (ascending row), else the n_extra members nearest to the centroid
 * (torch.cdist + topk(largest=False): ascending distance; equal distances -> lower row first). dist2 [T][K] fp32 as
 * cogs_kmeans_sqdist leaves it (squared distances order like distances), assign int64 [T]; out_idx int64 [K][n_extra]
 * (-1 padded), out_counts int32 [K] = min(members, n_extra). n_extra <= 8. */
cogs_status cogs_select_near_centroid(cogs_stream stream, const float* dist2, const int64_t* assign, int T, int K, int n_extra,
                                      int64_t* out_idx, int32_t* out_counts);
/* One k-means++ step (:46-60): squared distance of every row to feature row `row`, folded into nearest2 (device fp32 [T]:
 * first != 0 stores, else min). probs_host (pinned host fp32 [T], nullable): the updated nearest2 is copied there and the
 * stream is synchronised, so the caller can draw the next centre (torch.multinomial on the CPU generator) right away.
 * Workspace: cogs_kmeans_workspace_bytes(T, PD, 1). */
cogs_status cogs_kmeans_pp_step(cogs_stream stream, int dtype, const void* feats, int T, int64_t PD, int row, int first,
                                float* nearest2, float* probs_host, void* ws, size_t ws_bytes);
/* The whole k-means++ seeding (:41-62) in ONE call, no host round trip per centre. first_row = the first centre (the
 * caller's random.randint draw); idx (device int32 [K], all written): idx[0] = first_row, entry m the row drawn after m centres:
 * probs = (sqrt(nearest distance^2))^2 normalised by their sum, torch.multinomial(probs, 1) = argmax(probs / q), q ~
 * Exponential(1) (ATen's n_sample == 1 path) -- q_draws (device fp32 [K-1][T]) are those draws, made ahead on the
 * caller's CPU generator, one [T] row per centre, exactly as K - 1 multinomial calls would consume it. *zero_flag (device
 * int32) is set when a step finds every probability zero (the reference's random.randint branch, :57-59): the indices
 * are then not usable and the caller seeds step by step with cogs_kmeans_pp_step instead. nearest2: device fp32 [T]
 * scratch. The sum of the probabilities is taken in fp64 in a fixed order, not in torch's fp32 summation order: it is a
 * common divisor of all ratios. Workspace: cogs_kmeans_workspace_bytes(T, PD, 1). */
cogs_status cogs_kmeans_pp(cogs_stream stream, int dtype, const void* feats, int T, int64_t PD, int K, int first_row,
                           const float* q_draws, int32_t* idx, int32_t* zero_flag, float* nearest2, void* ws, size_t ws_bytes);
/* The whole Lloyd loop (:71-131) from given centres: per iteration distances -> assignment -> means / reseeds -> centre
 * shift, stopping after max_iter iterations or when the shift is <= tol. The library queues up to four iterations
 * between two synchronisations of the stream (it reads eight control words from host-mapped memory); every kernel of an
 * iteration queued behind the converged one returns without touching anything, so centres / assign are those of the
 * iteration the reference stops at. Empty clusters (:116-120: one random.randint(0, T-1) per empty cluster, ascending
 * cluster index, every iteration) take their rows from reseed_pool (HOST int32 [pool_len], pool_len <= 4096: the caller's
 * pre-drawn values, consumed in order, copied into host-mapped memory before the first launch; *reseeds_used reports how many). If an iteration
 * needs more than are left it is NOT committed: the call returns COGS_OK with *pool_exhausted = 1 and *iterations = the
 * completed ones; draw more and call again with the remaining iteration budget. T + K + 1 <= 16 384 (the assignments
 * and the cluster counters are staged in LDS). Workspace: cogs_kmeans_workspace_bytes(T, PD, K). */
cogs_status cogs_kmeans_lloyd(cogs_stream stream, int dtype, const void* feats, const float* ts, int T, int64_t PD, int K,
                              float alpha, int max_iter, float tol, const int32_t* reseed_pool, int pool_len,
                              float* centres, float* centre_ts, int64_t* assign, int* iterations, int* reseeds_used,
                              int* pool_exhausted, void* ws, size_t ws_bytes);
/* How close the assignments of the LAST cogs_kmeans_lloyd call on this workspace were (host outputs; synchronises).
 * Per row and iteration: the relative change of the row's feature distances that would flip the decision between its
 * best and second-best cluster -- with every time term equal this is (d2 - d1) / mean(d1, d2) of the two nearest feature
 * distances, the margin of the near-tie study; a decision the feature distances cannot flip is
 * +inf. *min_margin = the minimum over all rows and iterations, *rows_below = the number of (row, iteration) pairs
 * below 1e-3. Below that margin the reference's own torch.cdist rounding decides the row and no other summation order
 * reproduces it; at or above it the assignment equals the reference's. */
cogs_status cogs_kmeans_margins(cogs_stream stream, int T, int64_t PD, int K, void* ws, size_t ws_bytes, float* min_margin,
                                int32_t* rows_below);
/* dtype conversion / zero-padded row copy (features.to(float32), patch padding) */
cogs_status cogs_pack_rows(cogs_stream stream, int in_dtype, int out_dtype, const void* in, int64_t ld_in,
                           void* out, int64_t ld_out, int rows, int cols_in, int cols_out);

/* GPU pre-processing (image_processing_videollama3.py:235-347): uint8 frames [T,H,W,3] -> Pillow-exact bicubic
 * resize to (th,tw) -> value_table[c][byte] (fp32 [3,256], = rescale+normalize per byte) -> merge-window-major patch rows [T*(th/14)*(tw/14), 588] in out_dtype.
 * bounds_* [out,2] / coef_* [out,ks*] are Pillow's per-output tap tables (device int32; built on the host,
 * cogstream_amd.processing.resample_coeffs). ws >= T*H*tw*3 bytes. */
cogs_status cogs_preprocess_workspace_bytes(int T, int H, int tw, size_t* bytes);
cogs_status cogs_preprocess_frames(cogs_stream stream, const uint8_t* frames, int T, int H, int W, int th, int tw,
                                   int merge, const int32_t* bounds_x, const int32_t* coef_x, int ksx,
                                   const int32_t* bounds_y, const int32_t* coef_y, int ksy, const float* value_table,
                                   void* out, int out_dtype, void* ws, size_t ws_bytes);

/* logits post-processing (model/generation_config.json:2-12; qaselect_module_predict.py:86-103) */
/* cogs_argmax: the FIRST maximum under IEEE == (+0 == -0), 0 on a row of -inf. cogs_logits_process, in place: repetition
 * penalty (every id of prev once, whatever its multiplicity: s < 0 ? s * penalty : s / penalty), then the allowed-id mask
 * (n_allowed <= 256, else COGS_E_INVALID; everything else becomes -inf), then / temperature -- each ONE fp32 IEEE operation.
 * cogs_topk (1 <= top_k <= 1024, else COGS_E_INVALID): descending, equal values by ascending index; past the finite entries
 * the tail is (-inf, -1). */
cogs_status cogs_argmax(cogs_stream stream, const float* logits, int n, int64_t* out, void* ws /* >= 512 B */);
cogs_status cogs_logits_process(cogs_stream stream, float* logits, int n, const int64_t* prev, int n_prev,
                                float repetition_penalty, const int32_t* allowed, int n_allowed,
                                float temperature, float* tmp /* >= n_prev floats */);
cogs_status cogs_topk(cogs_stream stream, const float* logits, int n, int top_k, float* topk_val,
                      int32_t* topk_idx, float* ws /* >= n floats */);
/* Per-row log-sum-exp, target logit and first-maximum argmax of fp32 logits [rows, n] (row stride ld elements; n and ld
 * multiples of 4, `logits` 16-byte aligned): what F.cross_entropy(logits, targets, ignore_index=-100, reduction="none")
 * and logits.argmax(-1) read out of the logits of Qwen2ForCausalLM.forward (behind model/cogreasoner_chat.py:680-693,
 * 737-751); the log-probability of row r's target is target_logit[r] - lse[r]. targets (device int64 [rows], nullable):
 * -100 = ignored row; a target outside [0, n) cannot be refused without a synchronisation, so such a row is treated as
 * ignored and counted in *n_bad (device int32, nullable; set by the call). Outputs, each nullable: lse fp32 [rows] = log
 * sum_v exp(logit_v); target_logit fp32 [rows] (0 on ignored rows); argmax int64 [rows] (FIRST maximum, as torch.argmax /
 * cogs_argmax); max_logit fp32 [rows]. The matrix is walked in the panels cogs_lm_score uses (cogs_debug_get
 * "lm_score_last_rows" / "_cols" / "_split" / "_chunk" report them), every element read once; no floating-point atomics: the same
 * call gives the same bits. Workspace: 16 bytes per row + the column-split partials of one panel. */
cogs_status cogs_row_lse_workspace_bytes(int rows, int n, size_t* bytes);
cogs_status cogs_row_lse(cogs_stream stream, const float* logits, int rows, int n, int64_t ld, const int64_t* targets,
                         float* lse, float* target_logit, int64_t* argmax, float* max_logit, int32_t* n_bad, void* ws,
                         size_t ws_bytes);
/* Beam search selection (GenerationMixin._beam_search: log_probs + running_beam_scores, then torch.topk over the flattened
 * [num_beams * vocab] candidates): the k largest of v(r, t) = scores[r * ld + t] + row_add[r] (ONE fp32 addition; row_add
 * device fp32 [rows], NULL = +0) over rows x n, written in descending order of v as out_val / out_row / out_tok [k] (device);
 * equal values go by ascending flat index r * n + t. -inf scores are legal (the allowed-id mask) and rank last, in index order;
 * a sum of -0 counts and is reported as +0. NaN is NOT supported (a NaN score may be dropped or ranked anywhere).
 * 1 <= rows <= 16, 1 <= k <= 64, n <= 262144 (else COGS_E_UNSUPPORTED); k <= rows * n, n and ld multiples of 4, ld >= n, scores
 * 16-byte aligned (else COGS_E_INVALID). Every score is read once, no floating-point atomics (the same call gives the same
 * bits), no host synchronisation. ws >= cogs_beam_topk_workspace_bytes(rows, n, k). */
cogs_status cogs_beam_topk_workspace_bytes(int rows, int n, int k, size_t* bytes);
cogs_status cogs_beam_topk(cogs_stream stream, const float* scores, int rows, int n, int64_t ld, const float* row_add, int k,
                           float* out_val, int32_t* out_row, int32_t* out_tok, void* ws, size_t ws_bytes);
/* x[r * ld + i] -= sub[r] (fp32 [rows, n] in place; n and ld multiples of 4, x 16-byte aligned): logits -> log-probabilities
 * with sub = the rows' lse of cogs_row_lse. */
cogs_status cogs_sub_rows(cogs_stream stream, float* x, int rows, int n, int64_t ld, const float* sub);
/* One sampled token from a PROCESSED fp32 row (after cogs_logits_process's penalty / mask): TemperatureLogitsWarper
 * (v = scores / temperature, ONE fp32 IEEE division; temperature > 0, 1 = off) -> TopKLogitsWarper (top_k <= 0 or >= n: off;
 * keeps every v >= the k-th largest) -> TopPLogitsWarper (top_p >= 1: off; the ascending cumulative probability <= fp32(1 -
 * top_p) is dropped, the best token always stays, so top_p <= 0 keeps the best token only) -> softmax ->
 * torch.multinomial(probs, 1) = argmax_i probs_i / q_i, q ~ Exp(1), the lower id on equal scores (GenerationMixin._sample of
 * transformers 4.46.3 with model/generation_config.json:2-12; call site model/cogreasoner_chat.py:802-807). `draws`: NULL ->
 * q_i = -logf(u), u = ((x >> 8) + 1) 2^-24 with x the first word of Philox4x32-10 under counter (i, offset low word, offset
 * high word, 0) and key (seed low word, seed high word), no host round trip; else device float [n] holding the CPU generator's
 * exponential draws of this step (parity with the reference's CPU sampler). ws >= cogs_sample_workspace_bytes().
 * The contract where HF leaves the outcome to its unstable sort, by path (cogs_debug_get "sample_last_path"; the path is a
 * function of (n, top_k) alone):
 *  - path 1, 0 < top_k <= 64 and 64 top_k <= n <= 262144 (64 slices of ceil(n / 64) entries, then a merge): every entry tied
 *    with the k-th value is kept, as in HF. The kept list is ordered by descending v, equal v by ascending id, and top-p cuts
 *    it by position: the kept count is HF's, and a cut inside a block of equal v keeps the lower ids. Limits: a slice hands
 *    over at most top_k candidates and the list holds at most 1024 entries, so with more than top_k ties of the k-th value
 *    inside one slice, or more than 1024 kept, the surplus ties (highest ids first) are dropped; everything strictly above the
 *    k-th value is kept, nothing below it, and n_kept >= top_k.
 *  - path 2, every other (n, top_k) (one workgroup, radix selects): ties with the k-th value are all kept (HF), and so is
 *    every entry whose probability equals the top-p boundary probability -- on a tie at that boundary more than HF keeps.
 * Both: -0.0 counts as +0.0 (HF compares with IEEE <); entries at -inf (the allowed-id mask) are never kept, a row of nothing
 * but -inf gives token 0 and n_kept 0; NaN scores are NOT supported. Optional kept_idx / kept_prob [kept_cap] + n_kept (all
 * three and kept_cap > 0, or none) report the surviving ids and their renormalised probabilities: path 1 in the order above,
 * path 2 in any order. *n_kept is the FULL survivor count; only the first min(n_kept, kept_cap) entries are written (path 2:
 * any kept_cap of them). n <= 0, top_k < 0, temperature <= 0 or NaN, or an incomplete report triple: COGS_E_INVALID; path 1
 * without ws: COGS_E_WORKSPACE; in both cases nothing is written. */
size_t cogs_sample_workspace_bytes(void);
cogs_status cogs_sample(cogs_stream stream, const float* logits, int n, float temperature, int top_k, double top_p,
                        const float* draws,
                        uint64_t seed, uint64_t offset, int64_t* out_token, int32_t* kept_idx, float* kept_prob,
                        int32_t* n_kept, int kept_cap, void* ws);

/* ------------------------------------------------------------------ vision encoder ---- */

/* Packed ViT weights (borrowed device pointers, `dtype` elements). HF names (A18):
 * model.vision_encoder.{embeddings.patch_embedding, encoder.layers.N.*, post_layernorm}.
 * Packing done once at load (cogstream_amd/weights.py): patch_w [hidden, patch_pad] zero padded;
 * qkv_w [3*hidden, hidden] = q,k,v rows stacked, q/k rows of each head interleaved as rotary pairs;
 * fc1_w [inter_pad, hidden], fc1_b [inter_pad], fc2_w [hidden, inter_pad] zero padded.
 * LayerNorm folding (bf16 production path; both pointers non-NULL and hidden % 64 == 0): qkv_w / fc1_w then hold
 * the rows of W * diag(ln_gamma) with their mean over k removed -- every row sums to zero, see cogs_gemm_desc.ln_ab for
 * the exact contract -- and qkv_c / fc1_c [rows] fp32 = bias + W . ln_beta; the encoder then never materialises LN(x):
 * the GEMMs that write the residual stream emit per-row statistics and the QKV / fc1 GEMMs apply them in their epilogue.
 * With the pointers NULL (fp32 parity mode) qkv_w / fc1_w are the plain weights and LayerNorm runs as its own kernel. */
typedef struct {
    const void *ln1_g, *ln1_b, *qkv_w, *qkv_b, *o_w, *o_b, *ln2_g, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
    const float *qkv_c, *fc1_c;
} cogs_vit_layer;
typedef struct {
    int dtype;
    int hidden, inter_pad, layers, heads, patch_dim, patch_pad;
    float ln_eps;
    const void *patch_w, *patch_b, *post_ln_g, *post_ln_b;
    const cogs_vit_layer* layer; /* host array [layers], copied by cogs_vit_load */
} cogs_vit_weights;
cogs_status cogs_vit_load(cogs_handle h, const cogs_vit_weights* w);
cogs_status cogs_vit_workspace_bytes(cogs_handle h, int64_t n_patches, size_t* bytes);
/* Videollama3VisionEncoderModel.forward (modeling_videollama3_encoder.py:479-510).
 * pixel_values [N,588] (pix_dtype fp32 or bf16), grid_sizes host int64 [V,3] = (t,gh,gw),
 * merge_sizes host int64 [V]; out_tokens [M, hidden] in the weights' dtype. */
cogs_status cogs_vit_encode(cogs_handle h, cogs_stream stream, const void* pixel_values, int pix_dtype,
                            const int64_t* grid_sizes, const int64_t* merge_sizes, int V, int attn_mode,
                            void* out_tokens, void* ws, size_t ws_bytes);
/* cogs_vit_encode runs a clip of two or more frames as `streams` contiguous frame ranges on as many streams (the caller's
 * and up to three the handle owns; frames are independent under per-frame attention, the tokens are bit-identical to a
 * one-stream encode): one range's kernels fill the partly empty last rounds of another's persistent GEMM launches. The
 * ranges are queued layer by layer in turn, so every stream starts within one layer of the first. streams = 1 keeps
 * everything on the caller's stream, 2 is the default, 3 and 4 are allowed. */
cogs_status cogs_vit_set_streams(cogs_handle h, int streams);

/* ----------------------------------------------------------------------- multi-GPU ------ */

/* The one data-path collective of the path (the reference never shards a clip, its only
 * distributed code is init + per-video replicas, evaluate/answer_generate.py:155,186-187): frames of a clip are encoded
 * (and projected) by the ranks of one node, and ONE all-gather reassembles the visual tokens in frame order. Every rank
 * contributes `local_rows` rows of `row_bytes` bytes (equal counts: a ragged frame split pads to the largest shard);
 * `global` receives world * local_rows rows in rank order. `nccl_comm` is an ncclComm_t the caller created (rccl.h; one
 * process per GPU); the call enqueues ncclAllGather on `stream`. librccl.so is bound lazily with dlopen -- the library
 * has no link-time dependency on it -- and COGS_E_UNSUPPORTED is returned when it cannot be loaded. In-place use
 * (local == global + rank * local_rows * row_bytes) is allowed, as for ncclAllGather. The Python host does the same
 * through torch.distributed (cogstream_amd/parallel.py), whose "nccl" backend is RCCL. */
cogs_status cogs_allgather_tokens(cogs_stream stream, void* nccl_comm, const void* local, size_t local_rows,
                                  size_t row_bytes, void* global);

/* MlpGeluProjector (model/cogreasoner_chat.py:199-211): Linear -> GELU(erf) -> Linear */
typedef struct {
    int dtype; int in_dim, out_dim;
    const void *w1, *b1, *w2, *b2;
} cogs_proj_weights;
cogs_status cogs_proj_load(cogs_handle h, const cogs_proj_weights* w);
cogs_status cogs_project(cogs_handle h, cogs_stream stream, const void* tokens, int M, void* out, void* ws,
                         size_t ws_bytes /* >= M*out_dim elements */);
/* encode_images (model/cogreasoner_chat.py:264-276: vision_encoder, then mm_projector) as ONE call: cogs_vit_encode with the
 * projector's two GEMMs of every frame range queued behind that range's encoder on ITS stream, instead of on the caller's
 * stream after the join (round 6: the ranges' projections overlap the other ranges' last layers). out_tokens [M, hidden] is
 * still written (callers gather / cache the encoder tokens); proj_out [M, out_dim]; proj_ws >= M * out_dim elements.
 * Results are the bits of cogs_vit_encode followed by cogs_project. */
cogs_status cogs_vit_encode_project(cogs_handle h, cogs_stream stream, const void* pixel_values, int pix_dtype,
                                    const int64_t* grid_sizes, const int64_t* merge_sizes, int V, int attn_mode,
                                    void* out_tokens, void* ws, size_t ws_bytes, void* proj_out, void* proj_ws,
                                    size_t proj_ws_bytes);

/* ------------------------------------------------------------------------- Qwen2 ------ */

/* Packed Qwen2 weights. HF names: model.layers.N.{input_layernorm, self_attn.{q,k,v,o}_proj,
 * post_attention_layernorm, mlp.{gate,up,down}_proj}, model.norm, lm_head (untied).
 * qkv_w [(hq+2*hkv)*hd, hidden] with q/k head rows interleaved as rotary pairs, qkv_b likewise;
 * gu_w [2*inter, hidden] rows interleaved (gate_i, up_i); down_w [hidden, inter];
 * lm_head [vocab, hidden] (vocab % 4 == 0). */
typedef struct {
    const void *in_ln, *qkv_w, *qkv_b, *o_w, *post_ln, *gu_w, *down_w;
} cogs_llm_layer;
typedef struct {
    int dtype;
    int hidden, inter, layers, heads, kv_heads, head_dim, vocab;
    float rms_eps, rope_theta;
    const void *final_norm, *lm_head;
    const cogs_llm_layer* layer; /* host array [layers] */
} cogs_llm_weights;
cogs_status cogs_llm_load(cogs_handle h, const cogs_llm_weights* w);

/* e4m3 copies of the packed matrices of the loaded model (cogs_quantize_fp8_rows layout: codes [N][K] dense, scale [N]), in
 * the packing of cogs_llm_layer. While attached, a cogs_llm_forward / _segments over ONE token reads them through
 * cogs_gemv_fp8 instead of the matrices of cogs_llm_weights, and cogs_llm_decode_rows / _slots reads them through
 * cogs_gemm_rows_fp8; every other M > 1 GEMM and cogs_lm_score keep reading the latter,
 * which the caller has replaced by the dequantised values so that both evaluate one model. NULL detaches; cogs_llm_load
 * detaches too (the codes belong to one weight set). Needs hidden, inter and heads * head_dim to be multiples of 16.
 * Debug switches llm_decode_fp8 = 0 / llm_rows_fp8 = 0: single-token steps / the multi-row step go through the dequantised
 * matrices again (in-process A/B; the multi-row step gives the same bits either way);
 * cogs_debug_get("llm_last_decode_fp8") says what the last forward took, "llm_last_rows_fp8" what the last multi-row step. */
typedef struct {
    const uint8_t *qkv_q, *o_q, *gu_q, *down_q;
    const float *qkv_s, *o_s, *gu_s, *down_s;
} cogs_llm_fp8_layer;
typedef struct {
    int layers;
    const uint8_t* lm_head_q; const float* lm_head_s;
    const cogs_llm_fp8_layer* layer; /* host array [layers] */
} cogs_llm_fp8_weights;
cogs_status cogs_llm_attach_fp8(cogs_handle h, const cogs_llm_fp8_weights* w);

/* KV cache, caller-owned: k and v are [layers][max_len][kv_heads*head_dim] in the weights' dtype */
typedef struct {
    void* k; void* v;
    int max_len;
    int len;      /* tokens already cached; advanced by cogs_llm_forward */
} cogs_kv;
cogs_status cogs_llm_workspace_bytes(cogs_handle h, int max_tokens, int max_context, size_t* bytes);
/* One Qwen2Model forward over S new tokens given as embeddings [S, hidden] at positions
 * kv->len .. kv->len+S-1 (causal over cache + new tokens); kv == NULL: stateless forward
 * (event summaries, cogreasoner_chat.py:303-316). Outputs, each nullable:
 *   last_logits  fp32 [vocab]   lm_head(norm(h_last))          (generate / decode)
 *   pooled_mean  fp32 [hidden]  mean_t norm(h_t)                (cogreasoner_chat.py:317,323)
 *   hidden_out   [S, hidden]    norm(h)  (last_hidden_state) */
cogs_status cogs_llm_forward(cogs_handle h, cogs_stream stream, const void* embeds, int S, cogs_kv* kv,
                             float* last_logits, float* pooled_mean, void* hidden_out, void* ws,
                             size_t ws_bytes);

/* Lockstep decode of R (<= 16) continuations of ONE prompt: GenerationMixin.generate(num_return_sequences=R) behind
 * model/cogreasoner_chat.py:802-807 expands the prompt R times; here the prompt's KV rows [0, prefix_len) of k / v (the cogs_kv
 * layout) are shared and read once per step, and every sequence keeps only the rows it generated: tail_k / tail_v
 * [layers][R][tail_max][kv_heads * head_dim]. All rows stand at position prefix_len + tail_len. */
typedef struct {
    void* k; void* v; int max_len;   /* shared cache, as cogs_kv */
    int prefix_len;                  /* prompt rows every sequence sees */
    void* tail_k; void* tail_v;
    int tail_max;
    int tail_len;                    /* rows every sequence has generated; advanced by cogs_llm_decode_rows */
} cogs_kv_rows;
cogs_status cogs_llm_decode_rows_workspace_bytes(cogs_handle h, int R, int max_prefix, size_t* bytes);
/* One Qwen2 step over R new tokens, one per sequence, given as embeddings [R, hidden]: per layer RMSNorm, qkv
 * (cogs_gemm_rows; bias, rotary at the common position, pre-scaled Q), the new K / V rows into the tails, cogs_attention_rows,
 * o + residual, RMSNorm, gate / up SwiGLU, down + residual; then the final norm and the lm_head -> logits fp32 [R, vocab].
 * Every weight byte is read once per step. bf16 and head_dim 128 only (else COGS_E_UNSUPPORTED); hidden, inter and
 * heads * head_dim must be multiples of 64. With e4m3 codes attached (cogs_llm_attach_fp8) every GEMM of the step streams
 * the codes (cogs_gemm_rows_fp8: half the weight bytes, bit-identical logits); with the debug switch llm_rows_fp8 set to 0 it
 * reads the dequantised matrices of cogs_llm_weights. cogs_debug_get("llm_last_rows_fp8") says which;
 * "llm_last_decode_fp8" describes single-token cogs_llm_forward steps only and reads 0 after this call either way.
 * Row r's logits do not depend on the other rows. */
cogs_status cogs_llm_decode_rows(cogs_handle h, cogs_stream stream, const void* embeds, int R, cogs_kv_rows* kv,
                                 float* logits, void* ws, size_t ws_bytes);
/* The same step for beam search, where row r continues the sequence row parent[r] held one step ago: tail_slot (device int32
 * [R][tail_max], row stride tail_max; NULL = cogs_llm_decode_rows) names, per row and tail position, the slot whose tail holds
 * that position's K / V (cogs_attn_rows_desc.tail_slot). Row r's new K / V is still written at slot r, position tail_len: the
 * caller sets tail_slot[r][tail_len] = r before the step. Nothing is copied; cogs_kv_rows is unchanged. */
cogs_status cogs_llm_decode_rows_slots(cogs_handle h, cogs_stream stream, const void* embeds, int R, cogs_kv_rows* kv,
                                       const int32_t* tail_slot, float* logits, void* ws, size_t ws_bytes);

/* Teacher-forced scoring: the outputs of cogs_row_lse for logits = lm_head(hidden) WITHOUT the [S, vocab] logits --
 * Qwen2ForCausalLM.forward(labels=) / ForCausalLMLoss behind forward_train and forward (model/cogreasoner_chat.py:604-693,
 * 696-751), which materialise them (2.5 GB of fp32 for 4 096 tokens at vocab 152 064). hidden [S, hidden] in the weights'
 * dtype = cogs_llm_forward's hidden_out (with or without a KV cache); targets[i] = the token that FOLLOWS row i (the
 * caller shifts; -100 = ignore, out of range = ignored and counted in *n_bad); lse / target_logit / argmax / max_logit /
 * n_bad as for cogs_row_lse. The library walks row blocks x vocabulary panels: the lm_head GEMM writes one fp32 panel
 * (the accumulators last_logits comes from, not rounded to bf16), a fold kernel reduces it into 16 bytes of state per
 * row, the next panel overwrites it. cogs_lm_score_workspace_bytes does not grow with S * vocab: one panel of at most
 * 64 MiB (so that it stays in the 256 MiB Infinity Cache between the GEMM that writes it and the fold that reads it) +
 * 16 bytes per row + the partials of a column-split fold. S == 1 takes the GEMV of last_logits and gives cogs_argmax's
 * token for the same row. COGS_E_INVALID: S <= 0 or no LLM loaded; COGS_E_WORKSPACE: ws too small. */
cogs_status cogs_lm_score_workspace_bytes(cogs_handle h, int S, size_t* bytes);
cogs_status cogs_lm_score(cogs_handle h, cogs_stream stream, const void* hidden, int S, const int64_t* targets,
                          float* lse, float* target_logit, int64_t* argmax, float* max_logit, int32_t* n_bad,
                          void* ws, size_t ws_bytes);

/* nseg independent sequences stored back to back in embeds [S,H] (cu_seqlens_host [nseg+1], host memory, 0 .. S):
 * one stateless forward -- positions and causal attention restart at every sequence -- and the mean over each
 * sequence of the final hidden states -> pooled_means [nseg, H] fp32. Replaces the K sequential
 * self.get_model()(inputs_embeds=...).last_hidden_state.mean(dim=1) calls of select_events_based_on_summary
 * (model/cogreasoner_chat.py:303-322: one per event, one for the question). Synchronises the stream once (host
 * staging of the position table). Workspace: cogs_llm_workspace_bytes(h, S, S). */
cogs_status cogs_llm_forward_segments(cogs_handle h, cogs_stream stream, const void* embeds, int S,
                                      const int32_t* cu_seqlens_host, int nseg, float* pooled_means, void* ws,
                                      size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* COGS_H_ */
