// Internal launcher interface between the C-ABI layer (capi.hip, capi_vit.hip, capi_llm.hip) and the kernel files.
// Every launcher enqueues on the given stream, never synchronises, never allocates, and
// returns a COGS_* status (0 = ok).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "attn_plan.h"

#define COGS_ACT_NONE 0
#define COGS_ACT_GELU_TANH 1
#define COGS_ACT_GELU_ERF 2
#define COGS_ACT_SWIGLU 3

struct CogsGemm {
    int dtype = 0;                 // COGS_DT_*
    const void* A = nullptr; long lda = 0;   // [M,K], elements per row
    const void* W = nullptr; long ldw = 0;   // [N,K]
    void* C = nullptr; long ldc = 0;         // [M,N] (SWIGLU: [M,N/2])
    const void* bias = nullptr;              // [N]
    const void* residual = nullptr; long ldr = 0;
    int M = 0, N = 0, K = 0;
    int act = 0;
    int out_f32 = 0;
    const float* rope_cos = nullptr;         // [M, head_dim/2], or interleaved [M, head_dim/2, 2] when rope_sin == nullptr
    const float* rope_sin = nullptr;
    int rope_cols = 0;
    int head_dim = 0;
    int force_small_tile = 0;                // testing: always use the 128x128 kernel
    int co_streams = 1;                      // streams the caller feeds with GEMMs of this size at the same time (few-tile choice:
                                             //   the CUs a launch leaves idle are then not lost; cogs_vit_encode's two-stream mode: 2)
    const void* rms_gamma = nullptr;         // M == 1 only: RMS-normalise A on the fly with this weight
    float rms_eps = 0.f;
    // M == 1 only: output columns [kv_col0, kv_col0 + kv_dim) go to kv_k[0..kv_dim), the next kv_dim to kv_v
    // (single-token decode writes the new K/V row straight into the cache; no kv_append launch)
    void* kv_k = nullptr; void* kv_v = nullptr; int kv_col0 = 0; int kv_dim = 0;
    // rope epilogues only: columns [0, q_cols) (the Q heads) are multiplied by q_scale before rounding
    float q_scale = 1.f; int q_cols = 0;
    // optional 2-D rotary LUT (ViT): rope_lut [maxpos][head_dim/4][2] fp32 = (cos, sin) of pos*inv_freq[f], rope_rowpos
    // [M] = h | w << 16. The ping-pong kernel keeps the LUT in LDS and reads the factors from there (first half of a
    // head's pairs rotates with h, second half with w); rope_cos must still be the matching per-row table.
    const float* rope_lut = nullptr; const int* rope_rowpos = nullptr; int rope_maxpos = 0;
    // LayerNorm fused around the GEMM (gemm_epilogue.h EPI_ROWSTAT / EPI_LNFOLD; bf16 kernels):
    float* row_stats = nullptr;              // != null: also write per-row partial (sum, sum of squares) of the outputs,
                                             //   [M][N/64][2] fp32 (N % 64 == 0)
    // head-major output (gemm_epilogue.h EPI_HM; bf16, rotary epilogues): hm_rows > 0 = rows of the whole output buffer, C is
    // [N / hm_cols][hm_cols / head_dim][hm_rows][head_dim] instead of [M][N] (ldc ignored); M <= hm_rows rows are written
    long hm_rows = 0; int hm_cols = 0;
    const float* ln_ab = nullptr;            // != null: y = ln_ab[r][0] * acc + col_c[n] instead of acc + bias. W = rows of
    const float* col_c = nullptr;            //   W0*diag(gamma) made ZERO-SUM over k, col_c = bias + W0.beta; bias must be null
                                             //   (include/cogs.h, cogs_gemm_desc.ln_ab, has the contract)
};
int cogs_k_gemm(hipStream_t st, const CogsGemm& g);
// gemv_fp8.hip: M = 1 with W = OCP e4m3fn codes [N][ldw bytes] and one power-of-two fp32 scale per row; every other field as
// for the GEMV behind cogs_k_gemm (rms_gamma, kv_k / kv_v, q_scale included); g.dtype = the activations' type
int cogs_k_gemv_fp8(hipStream_t st, const CogsGemm& g, const float* scale);
// rows of w [N][ldw] (bf16 / fp32) -> codes [N][ldq bytes], scale [N] = 2^ceil(log2(absmax / 448)) (1 for a zero row);
// deq != null: also the dequantised rows in w's type (deq may be w)
int cogs_k_quantize_fp8_rows(hipStream_t st, int dtype, const void* w, long ldw, int N, int K, uint8_t* codes, long ldq,
                             float* scale, void* deq, long ldd);
// (a, b) = (rstd, -rstd * mean) per row from the EPI_ROWSTAT partials [rows][tiles][2]: ab [rows][2]
int cogs_k_ln_finalize(hipStream_t st, const float* stat_part, int rows, int tiles, int H, float eps, float* ab);

struct CogsAttn {
    int dtype = 0;
    const void* Q = nullptr; const void* K = nullptr; const void* V = nullptr; void* O = nullptr;
    long ldq = 0, ldk = 0, ldv = 0, ldo = 0;
    const int* cu_seqlens = nullptr;  // device [nseg+1]; block-diagonal segments (q and k alike)
    int nseg = 1;
    int max_seqlen = 0;
    const int* row_lo = nullptr;      // device [q_len]: same-segment key range, enables the
    const int* row_hi = nullptr;      //   "global attention + bias" mode of the eager reference
    float bias = 0.f;
    int q_len = 0, kv_len = 0;
    int hq = 1, hkv = 1, head_dim = 0;
    float scale = 1.f;
    int causal = 0;
    int q_pos0 = 0;
    int force_rowwise = 0;
    int nsplit = 1;                   // >1: split the keys over blocks (decode); needs ws
    void* ws = nullptr;               // cogs_attn_split_ws_bytes(nsplit, q_len, hq, head_dim) (attn_plan.h)
    size_t ws_bytes = 0;
    int q_prescaled = 0;              // Q already multiplied by scale*log2(e) (bf16 MFMA kernels only; no bias mode)
    int uniform_seqlen = 0;           // internal hint: > 0 = every cu_seqlens segment has exactly this many rows, in order
    long head_stride = 0;             // > 0: head-major Q / K / V (include/cogs.h cogs_attn_desc.head_stride); ViT kernel only
};
// cogs_k_attention / cogs_k_attention_rows snapshot the plan switches once (cogs_k_attention_tuning), take the plan of attn_plan.h and
// launch it; the launchers that take an AttnPlan are their halves in the other kernel files and launch what that plan says
AttnTuning cogs_k_attention_tuning();     // attn.hip: the plan switches of debug.h as they are now
int cogs_k_attention_vit(hipStream_t st, const struct CogsAttn& a, const AttnPlan& plan);   // attn_vit.hip: block-diagonal, hd 72, pre-scaled Q
int cogs_k_attention_decode(hipStream_t st, const struct CogsAttn& a, const AttnPlan& plan, float* part_o, float* part_ml);   // attn_decode.hip: one query row, hd 128, key-split partials
int cogs_k_attention(hipStream_t st, const CogsAttn& a);
// lockstep decode of `rows` sequences over one prompt (include/cogs.h cogs_attn_rows_desc): bf16, hd 128, pre-scaled Q
struct CogsAttnRows {
    const void* Q = nullptr; long ldq = 0;                       // [rows][hq * 128]
    const void* K = nullptr; const void* V = nullptr; long ldk = 0, ldv = 0; int prefix_len = 0;   // shared keys
    const void* tail_k = nullptr; const void* tail_v = nullptr;  // [rows][..][hkv * 128]: row r's own keys [0, tail_len)
    long tail_ld = 0, tail_row = 0; int tail_len = 0;            //   key stride, stride between rows (elements)
    void* O = nullptr;                                           // dense [rows][hq * 128]
    int rows = 0, hq = 1, hkv = 1, head_dim = 0;
    int nsplit = 1;                                              // splits of the shared keys (<= 127)
    void* ws = nullptr; size_t ws_bytes = 0;                     // cogs_attn_split_ws_bytes(nsplit + 1, rows, hq, head_dim) (attn_plan.h)
    const int32_t* tail_slot = nullptr; long tail_slot_ld = 0;   // non-null: row r's tail key j lives in tail slot tail_slot[r * ld + j]
};
int cogs_k_attention_decode_rows(hipStream_t st, const CogsAttnRows& a, const AttnPlan& plan, float* part_o, float* part_ml);   // attn_decode.hip: partials
int cogs_k_attention_combine(hipStream_t st, const AttnPlan& plan, const float* part_o, const float* part_ml, int q_len, int heads,
                             int head_dim, void* O, long ldo);   // attn.hip: plan.parts <= 128 partials of q_len x heads slots -> bf16 O
int cogs_k_attention_rows(hipStream_t st, const CogsAttnRows& a);     // both of the above
// gemm_rows.hip: bf16, 1 <= M <= 16, weights streamed once as the MFMA operand (not reachable through cogs_k_gemm: its plan is pinned)
int cogs_k_gemm_rows(hipStream_t st, const CogsGemm& g);
// the same with W = OCP e4m3fn codes [N][ldw bytes] and one power-of-two fp32 scale per row (ldw % 16 == 0): the bits of
// cogs_k_gemm_rows on the dequantised matrix code * scale
int cogs_k_gemm_rows_fp8(hipStream_t st, const CogsGemm& g, const float* scale);
long cogs_k_gemm_launch_count();   // kernels launched by cogs_k_gemm so far in this process


// norms
int cogs_k_layernorm(hipStream_t st, int dtype, const void* x, void* y, const void* gamma, const void* beta,
                     int rows, int H, float eps);
int cogs_k_rmsnorm(hipStream_t st, int dtype, const void* x, void* y, const void* gamma, int rows, int H, float eps);
// y[r] = mean_{i<group} LN(x[group*r+i])   (post_layernorm + 2x2 bilinear merge)
int cogs_k_ln_merge(hipStream_t st, int dtype, const void* x, void* y, const void* gamma, const void* beta,
                    int out_rows, int group, int H, float eps);

// vision front-end helpers
int cogs_k_pack_rows(hipStream_t st, int in_dtype, int out_dtype, const void* in, long ld_in, void* out,
                     long ld_out, int rows, int cols_in, int cols_out);
int cogs_k_vit_rope_table(hipStream_t st, float* cos_t, float* sin_t, int row0, int t, int gh, int gw, int ms,
                          const float* inv_freq, int n_freq);
// cu_seqlens[frame0+1 .. frame0+t] (and cu[0] for the first video) + optional same-frame row ranges, on the device
int cogs_k_vit_segments(hipStream_t st, int* cu, int* lo, int* hi, int row0, int frame0, int t, int per);
// pos[i] = i - cu[segment(i)]
int cogs_k_seg_positions(hipStream_t st, const int* cu, int nseg, int* pos);
int cogs_k_vit_rope_lut(hipStream_t st, int* rowpos, int row0, int t, int gh, int gw, int ms, float* lut, int maxpos,
                        const float* inv_freq, int n_freq);
int cogs_k_llm_rope_table(hipStream_t st, float* cos_t, float* sin_t, const int* pos, int pos0, int rows,
                          const float* inv_freq, int n_freq);

// GPU pre-processing: Pillow-exact bicubic resize + normalise + patchify (tmp: T*H*tw*3 bytes)
int cogs_k_preprocess(hipStream_t st, const uint8_t* frames, int T, int H, int W, int th, int tw, int ms,
                      const int* bx, const int* kx, int ksx, const int* by, const int* ky, int ksy, void* out,
                      int out_dtype, const float* table, uint8_t* tmp);

// token compression
int cogs_k_pixdiff_mask(hipStream_t st, int dtype, const void* pix, int t, int tokens_per_frame, int row_elems,
                        float thr, int min_tokens, uint8_t* mask);
int cogs_k_mask_fix(hipStream_t st, uint8_t* mask, int t, int tokens_per_frame, int min_tokens, const uint8_t* minor);
int cogs_k_frame_mean_to_slot0(hipStream_t st, int dtype, void* feats, int P, int D, const int* frames, int n_frames);
int cogs_k_gather_rows(hipStream_t st, int dtype, const void* table_a, const void* table_b, const int64_t* idx,
                       void* out, int rows, int D);
int cogs_k_mean_rows(hipStream_t st, int dtype, const void* x, long ldx, int rows, int D, float* out);
int cogs_k_cosine(hipStream_t st, const float* a, const float* b, int n, int D, float* out);

// time-aware k-means
int cogs_k_kmeans_sqdist(hipStream_t st, int dtype, const void* feats, int T, long PD, const float* centres,
                         const int* centre_rows, int K, float* ws, int nslices, float* dist2);
int cogs_k_kmeans_pp_step(hipStream_t st, int dtype, const void* feats, int T, long PD, int row, int first,
                          float* nearest2, float* probs_host, float* ws, int nslices);
int cogs_k_kmeans_pp(hipStream_t st, int dtype, const void* feats, int T, long PD, int K, int first_row, const float* q, int* idx,
                     int* zero_flag, float* nearest2, float* ws, int nslices);
int cogs_k_kmeans_margins(hipStream_t st, int T, long PD, int K, float* ws, float* min_margin, int* rows_below);
int cogs_k_kmeans_lloyd(hipStream_t st, int dtype, const void* feats, const float* ts, int T, long PD, int K, float alpha,
                        int max_iter, float tol, const int* pool_host, int pool_len, float* centres, float* centre_ts,
                        int64_t* assign, int* iterations, int* reseeds_used, int* exhausted, float* ws, int nslices);
size_t cogs_k_kmeans_ws(int T, long PD, int K, int* nslices);
int cogs_k_kmeans_assign(hipStream_t st, const float* dist2, const float* ts, const float* centre_ts, int T, int K,
                         float alpha, int64_t* assign, int* counts);
int cogs_k_kmeans_update(hipStream_t st, int dtype, const void* feats, const float* ts, int T, long PD, int K,
                         const int64_t* assign, const int* reseed_rows, float* centres, float* centre_ts,
                         float* ws, int nblk, float* shift_out);
int cogs_k_kmeans_update_blocks(long PD);
int cogs_k_select_near(hipStream_t st, const float* dist2, const int64_t* assign, int T, int K, int n, int64_t* picks,
                       int* counts);

// LLM helpers
// append S rows of K and V (adjacent column blocks of the fused qkv buffer) to the two caches in one launch
int cogs_k_kv_append(hipStream_t st, int dtype, const void* k_src, const void* v_src, long ld_src, void* k_dst,
                     void* v_dst, long ld_dst, int rows, int cols);
int cogs_k_copy_cols(hipStream_t st, int dtype, const void* src, long ld_src, void* dst, long ld_dst, int rows, int cols);
int cogs_k_argmax(hipStream_t st, const float* logits, int n, int64_t* out, float* ws);
// HF logits processors on one fp32 row: repetition penalty over `prev` (gather-then-scatter, so
// duplicates are penalised once), allowed-id mask (others -> -inf), temperature; `tmp` >= n_prev floats
int cogs_k_logits_process(hipStream_t st, float* logits, int n, const int64_t* prev, int n_prev, float rep_penalty,
                          const int32_t* allowed, int n_allowed, float temperature, float* tmp);
// the top_k largest logits in descending order (ties: lower index first); ws >= 2*n floats
int cogs_k_topk(hipStream_t st, const float* logits, int n, int top_k, float* topk_val, int32_t* topk_idx, float* ws);
// TopK -> TopP -> softmax -> multinomial of one processed fp32 row (sample.hip); ws >= cogs_k_sample_ws() bytes
size_t cogs_k_sample_ws();
int cogs_k_sample(hipStream_t st, const float* logits, int n, float temperature, int top_k, double top_p, const float* draws, uint64_t seed,
                  uint64_t offset, int64_t* out_token, int32_t* kept_idx, float* kept_prob, int* n_kept, int kept_cap,
                  void* ws);

// beam search (beam.hip): the k largest of scores[r][t] + row_add[r] over rows x n, descending, ties by ascending r * n + t
int cogs_k_beam_topk_ws(int rows, int n, int k, size_t* bytes);
int cogs_k_beam_topk(hipStream_t st, const float* scores, int rows, int n, long ld, const float* row_add, int k, float* out_val,
                     int32_t* out_row, int32_t* out_tok, void* ws, size_t ws_bytes);
int cogs_k_sub_rows(hipStream_t st, float* x, int rows, int n, long ld, const float* sub);   // x[r][:] -= sub[r]

// teacher-forced scoring (lm_score.hip): a [rows, n] fp32 logits matrix is walked as rows_b x cols_p panels; every panel is
// folded into 16 bytes of per-row state (maximum, sum of exp, first-maximum column); the last call writes the outputs
struct CogsLsePlan {
    int rows_b, cols_p;      // panel shape (rows_b * cols_p * 4 <= 64 MiB)
    int chunk, nsplit;       // columns per workgroup of the fold, workgroups per row of a full panel
    size_t state_bytes, part_bytes, panel_bytes;
};
void cogs_k_lse_plan(int rows, int n, CogsLsePlan* p);
// panel: fp32 [rows <= rows_b][ld] holding vocabulary columns [col0, col0 + width); col0 == 0 starts a row's state afresh.
// targets / target_logit / state: already offset to the panel's first row; part: rows_b * nsplit * 16 bytes (nsplit > 1)
int cogs_k_lse_fold(hipStream_t st, const CogsLsePlan& p, const float* panel, long ld, int rows, int width, int col0,
                    const int64_t* targets, float* target_logit, void* state, void* part);
int cogs_k_lse_final(hipStream_t st, const void* state, int rows, int n, const int64_t* targets, float* lse,
                     float* target_logit, int64_t* argmax, float* max_logit, int* n_bad);
