// C-ABI layer of libcogs_hip.so (see include/cogs.h): the handle, status / version strings, the debug switches, profiling
// and the thin per-operator entry points. The per-model launch sequences: capi_vit.hip (ViT encoder, projector, token
// all-gather) and capi_llm.hip (Qwen2 forward, multi-row decode, scoring); shared host pieces: capi_internal.h. No torch
// types, no exceptions, no stream synchronisation (host tables travel through a pinned, event-guarded ring).
#include "capi_internal.h"

#include <new>

CogsDebug g_cogs_debug;

// copy `bytes` of host data to the device on `st` through the handle's pinned ring (no stream synchronisation)
int stage_h2d(cogs_ctx* c, hipStream_t st, void* dst, const void* src, size_t bytes) {
    const int s = c->stage_next;
    c->stage_next = (s + 1) % cogs_ctx::STAGE_SLOTS;
    if (c->stage_busy[s]) {
        if (hipEventSynchronize(c->stage_ev[s]) != hipSuccess) return COGS_E_HIP;
        c->stage_busy[s] = false;
    }
    if (c->stage_cap[s] < bytes) {
        if (c->stage_host[s]) (void)hipHostFree(c->stage_host[s]);
        c->stage_host[s] = nullptr; c->stage_cap[s] = 0;
        const size_t cap = bytes < 4096 ? 4096 : bytes * 2;
        if (hipHostMalloc(&c->stage_host[s], cap, hipHostMallocDefault) != hipSuccess) return COGS_E_HIP;
        c->stage_cap[s] = cap;
    }
    if (!c->stage_ev[s] && hipEventCreateWithFlags(&c->stage_ev[s], hipEventDisableTiming) != hipSuccess) return COGS_E_HIP;
    memcpy(c->stage_host[s], src, bytes);
    if (hipMemcpyAsync(dst, c->stage_host[s], bytes, hipMemcpyHostToDevice, st) != hipSuccess) return COGS_E_HIP;
    if (hipEventRecord(c->stage_ev[s], st) != hipSuccess) return COGS_E_HIP;
    c->stage_busy[s] = true;
    return COGS_OK;
}

LseScratch lse_scratch(const CogsLsePlan& p, bool with_panel, void* base) {
    Carver c(base);
    void* state = c.take(p.state_bytes);
    void* part = p.part_bytes ? c.take(p.part_bytes) : nullptr;
    float* panel = with_panel ? (float*)c.take(p.panel_bytes) : nullptr;
    return {state, part, panel, c.off};
}
void lse_report(const CogsLsePlan& p) {
    g_cogs_debug.lm_score_last_split = p.nsplit;
    g_cogs_debug.lm_score_last_chunk = p.chunk;
    g_cogs_debug.lm_score_last_rows = p.rows_b;
    g_cogs_debug.lm_score_last_cols = p.cols_p;
}

static CogsGemm to_gemm(const cogs_gemm_desc* d) {
    CogsGemm g;
    g.dtype = d->dtype;
    g.A = d->A; g.lda = d->lda; g.W = d->W; g.ldw = d->ldw; g.C = d->C; g.ldc = d->ldc;
    g.bias = d->bias; g.residual = d->residual; g.ldr = d->ldr;
    g.M = d->M; g.N = d->N; g.K = d->K; g.act = d->act; g.out_f32 = d->out_f32;
    g.rope_cos = d->rope_cos; g.rope_sin = d->rope_sin; g.rope_cols = d->rope_cols; g.head_dim = d->head_dim;
    g.rope_lut = d->rope_lut; g.rope_rowpos = d->rope_rowpos; g.rope_maxpos = d->rope_maxpos;
    g.row_stats = d->row_stats; g.ln_ab = d->ln_ab; g.col_c = d->col_c;
    g.hm_rows = d->hm_rows; g.hm_cols = d->hm_cols;
    return g;
}

extern "C" {

const char* cogs_status_string(cogs_status s) {
    switch (s) {
        case COGS_OK: return "ok";
        case COGS_E_INVALID: return "invalid argument";
        case COGS_E_HIP: return "HIP runtime error";
        case COGS_E_UNSUPPORTED: return "unsupported configuration";
        case COGS_E_WORKSPACE: return "workspace missing or too small";
        default: return "unknown status";
    }
}

// 0.2: cogs_gemm_desc.hm_rows / hm_cols, cogs_attn_desc.head_stride; 0.3: cogs_lm_score, cogs_row_lse;
// 0.4: cogs_gemv_fp8, cogs_quantize_fp8_rows, cogs_llm_attach_fp8
const char* cogs_version(void) { return "cogstream_amd 0.4 (gfx950)"; }

// ---------------------------------------------------------------- diagnostics (csrc/debug.h)
// accepted range of a switch: on / off unless listed here
static bool cogs_debug_value_ok(const char* name, int64_t v) {
    struct Range { const char* name; int64_t lo, hi; };
    static const Range ranges[] = {
        {"gemm_wgs", 0, 256}, {"gemm_pad_pct", 100, 400}, {"gemm_group_m", 0, 64}, {"gemm_co_streams", 0, 8},
        {"gemm_ring_cost_permille", 1, 4000}, {"gemv_small_n", 0, 1 << 30}, {"gemv_fp8_load", 8, 16}, {"attn_vit", 0, 2}, {"attn_uniform_hint", 0, 1 << 20},
        {"attn_nq", 0, 2}, {"vit_split_max", 0, INT64_MAX}, {"llm_split_keys", 0, 1 << 24}, {"km_row_groups", 0, 1 << 16},
        {"lm_score_rows", 1, 1 << 16}, {"lm_score_cols", 0, 1 << 24}, {"lm_score_split", 0, 4096},
    };
    if (strcmp(name, "gemv_fp8_load") == 0 && v != 8 && v != 16) return false;
    for (const Range& r : ranges)
        if (strcmp(name, r.name) == 0) return v >= r.lo && v <= r.hi;
    return v == 0 || v == 1;
}

cogs_status cogs_debug_set(const char* name, int64_t value) {
    if (!name) return COGS_E_INVALID;
    if (!cogs_debug_value_ok(name, value)) return COGS_E_INVALID;
    if (value != 0 && (strcmp(name, "gemm_nostore") == 0 || strcmp(name, "gemm_trace") == 0))
        fprintf(stderr, "[cogs] debug switch %s = %lld: a timing / tracing mode -- cogs_gemm %s until it is set back to 0\n", name,
                (long long)value, strcmp(name, "gemm_nostore") == 0 ? "does NOT write its result" : "synchronises and prints per-tile stamps");
#define COGS_DBG_SET(n, dflt, doc) if (strcmp(name, #n) == 0) { g_cogs_debug.n = value; return COGS_OK; }
    COGS_DEBUG_SWITCHES(COGS_DBG_SET)
#undef COGS_DBG_SET
    return COGS_E_INVALID;
}

cogs_status cogs_debug_get(const char* name, int64_t* value) {
    if (!name || !value) return COGS_E_INVALID;
#define COGS_DBG_GET(n, dflt, doc) if (strcmp(name, #n) == 0) { *value = g_cogs_debug.n; return COGS_OK; }
    COGS_DEBUG_SWITCHES(COGS_DBG_GET)
#undef COGS_DBG_GET
    if (strcmp(name, "gemm_last_body") == 0) { *value = g_cogs_debug.gemm_last_body; return COGS_OK; }
    if (strcmp(name, "attn_last_kernel") == 0) { *value = g_cogs_debug.attn_last_kernel; return COGS_OK; }
    if (strcmp(name, "attn_vit_last_end") == 0) { *value = g_cogs_debug.attn_vit_last_end; return COGS_OK; }
    if (strcmp(name, "lm_score_last_split") == 0) { *value = g_cogs_debug.lm_score_last_split; return COGS_OK; }
    if (strcmp(name, "lm_score_last_chunk") == 0) { *value = g_cogs_debug.lm_score_last_chunk; return COGS_OK; }
    if (strcmp(name, "lm_score_last_rows") == 0) { *value = g_cogs_debug.lm_score_last_rows; return COGS_OK; }
    if (strcmp(name, "lm_score_last_cols") == 0) { *value = g_cogs_debug.lm_score_last_cols; return COGS_OK; }
    if (strcmp(name, "llm_last_decode_fp8") == 0) { *value = g_cogs_debug.llm_last_decode_fp8; return COGS_OK; }
    if (strcmp(name, "llm_last_rows_fp8") == 0) { *value = g_cogs_debug.llm_last_rows_fp8; return COGS_OK; }
    if (strcmp(name, "sample_last_path") == 0) { *value = g_cogs_debug.sample_last_path; return COGS_OK; }
    return COGS_E_INVALID;
}

const char* cogs_debug_list(void) {
    return
#define COGS_DBG_DOC(n, dflt, doc) #n " = " #dflt ": " doc "\n"
        COGS_DEBUG_SWITCHES(COGS_DBG_DOC)
#undef COGS_DBG_DOC
        "gemm_last_body (read only): body the last cogs_gemm dispatched to -- 1 128x128, 2 256x128 ring, 3 K-tile ping-pong, "
        "4 whole-line ping-pong, 5 ping-pong + ring (split launch), 6 GEMV\n"
        "attn_last_kernel (read only): kernel of the last cogs_attention -- 1 general MFMA, 2 ViT unpipelined, 3 ViT pipelined, "
        "4 single-token decode, 5 prompt LDS-DMA, 7 row-wise fp32, 8 ViT pipelined on head-major K/V\n"
        "attn_vit_last_end (read only): ragged end of the last pipelined ViT attention launch -- 10 x tiles behind the four-tile loop + "
        "32-key blocks of the last tile (41 .. 72: compile-time shape), 0 the run-time form\n"
        "lm_score_last_split / lm_score_last_chunk / lm_score_last_rows / lm_score_last_cols (read only): the last cogs_lm_score / "
        "cogs_row_lse -- workgroups per row of a full panel in the fold kernel (1: no column split), columns per workgroup, rows and "
        "columns of a panel\n"
        "llm_last_decode_fp8 (read only): 1 the last cogs_llm_forward / cogs_llm_forward_segments took the e4m3 GEMVs, 0 the weights' own type "
        "(single-token forwards only: the multi-row step sets it to 0 and reports in llm_last_rows_fp8)\n"
        "llm_last_rows_fp8 (read only): 1 the last cogs_llm_decode_rows / cogs_llm_decode_rows_slots streamed the attached e4m3 codes "
        "(cogs_gemm_rows_fp8), 0 the (dequantised) matrices of cogs_llm_weights\n"
        "sample_last_path (read only): path of the last cogs_sample -- 1 slice top-k + merge (0 < top_k <= 64, 64 top_k <= n <= 262144), "
        "2 whole-row radix selects\n";
}

cogs_status cogs_create(int device, cogs_handle* out) {
    if (!out) return COGS_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return COGS_E_HIP;
    cogs_ctx* c = new (std::nothrow) cogs_ctx();
    if (!c) return COGS_E_HIP;
    c->device = device;
    *out = c;
    return COGS_OK;
}

cogs_status cogs_profile_begin(cogs_handle h) {
    if (!h) return COGS_E_INVALID;
    h->prof_on = true;
    h->prof_used = 0;
    return COGS_OK;
}

cogs_status cogs_profile_end(cogs_handle h, cogs_stream stream, float* ms_per_class, int* launches_per_class) {
    if (!h || !ms_per_class || !launches_per_class) return COGS_E_INVALID;
    h->prof_on = false;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return COGS_E_HIP;
    for (int i = 0; i < COGS_PROF_CLASSES; ++i) { ms_per_class[i] = 0.f; launches_per_class[i] = 0; }
    for (size_t i = 0; i < h->prof_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->prof_ev[2 * i], h->prof_ev[2 * i + 1]) != hipSuccess) return COGS_E_HIP;
        const int cls = h->prof_cls[i];
        if (cls >= 0 && cls < COGS_PROF_CLASSES) { ms_per_class[cls] += ms; launches_per_class[cls] += i < h->prof_n.size() ? h->prof_n[i] : 1; }
    }
    h->prof_used = 0;
    return COGS_OK;
}

cogs_status cogs_destroy(cogs_handle h) {
    if (!h) return COGS_OK;
    for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
    for (int i = 0; i < cogs_ctx::STAGE_SLOTS; ++i) {
        if (h->stage_ev[i]) { (void)hipEventSynchronize(h->stage_ev[i]); (void)hipEventDestroy(h->stage_ev[i]); }
        if (h->stage_host[i]) (void)hipHostFree(h->stage_host[i]);
    }
    if (h->vit_inv_freq) (void)hipFree(h->vit_inv_freq);
    if (h->llm_inv_freq) (void)hipFree(h->llm_inv_freq);
    for (hipStream_t s2 : h->aux_streams) { (void)hipStreamSynchronize(s2); (void)hipStreamDestroy(s2); }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (hipEvent_t e : h->ev_joins) (void)hipEventDestroy(e);
    delete h;
    return COGS_OK;
}

// ---------------------------------------------------------------- operator level

cogs_status cogs_gemm(cogs_stream stream, const cogs_gemm_desc* d) {
    if (!d || !d->A || !d->W || !d->C) return COGS_E_INVALID;
    if (d->ln_ab && d->bias) return COGS_E_INVALID;     // col_c already contains the bias
    return cogs_k_gemm((hipStream_t)stream, to_gemm(d));
}

cogs_status cogs_gemm_rows(cogs_stream stream, const cogs_gemm_desc* d, float q_scale, int q_cols) {
    if (!d || !d->A || !d->W || !d->C) return COGS_E_INVALID;
    CogsGemm g = to_gemm(d);
    if (q_scale != 0.f) { g.q_scale = q_scale; g.q_cols = q_cols; }
    return cogs_k_gemm_rows((hipStream_t)stream, g);
}

cogs_status cogs_gemm_rows_fp8(cogs_stream stream, const cogs_gemm_desc* d, const float* scale, float q_scale, int q_cols) {
    if (!d || !d->A || !d->W || !d->C || !scale) return COGS_E_INVALID;
    CogsGemm g = to_gemm(d);
    if (q_scale != 0.f) { g.q_scale = q_scale; g.q_cols = q_cols; }
    return cogs_k_gemm_rows_fp8((hipStream_t)stream, g, scale);
}

cogs_status cogs_gemm_fused(cogs_stream stream, const cogs_gemm_desc* d, const cogs_gemm_fused_args* a) {
    if (!d || !a || !d->A || !d->W || !d->C) return COGS_E_INVALID;
    if (d->ln_ab && d->bias) return COGS_E_INVALID;     // as cogs_gemm
    CogsGemm g = to_gemm(d);
    if (a->q_scale != 0.f) { g.q_scale = a->q_scale; g.q_cols = a->q_cols; }
    g.rms_gamma = a->rms_gamma; g.rms_eps = a->rms_eps;
    g.kv_k = a->kv_k; g.kv_v = a->kv_v; g.kv_col0 = a->kv_col0; g.kv_dim = a->kv_dim;
    return cogs_k_gemm((hipStream_t)stream, g);
}

cogs_status cogs_attention_rows(cogs_stream stream, const cogs_attn_rows_desc* d) {
    if (!d || !d->Q || !d->K || !d->V || !d->tail_k || !d->tail_v || !d->O) return COGS_E_INVALID;
    if (d->dtype != COGS_DT_BF16) return COGS_E_UNSUPPORTED;
    CogsAttnRows a;
    a.Q = d->Q; a.ldq = d->ldq; a.K = d->K; a.V = d->V; a.ldk = d->ldk; a.ldv = d->ldv; a.prefix_len = d->prefix_len;
    a.tail_k = d->tail_k; a.tail_v = d->tail_v; a.tail_ld = d->tail_ld; a.tail_row = d->tail_row_stride; a.tail_len = d->tail_len;
    a.O = d->O; a.rows = d->rows; a.hq = d->hq; a.hkv = d->hkv; a.head_dim = d->head_dim;
    a.nsplit = d->nsplit > 1 ? d->nsplit : 1; a.ws = d->ws; a.ws_bytes = d->ws_bytes;
    a.tail_slot = d->tail_slot; a.tail_slot_ld = d->tail_slot_ld;
    return cogs_k_attention_rows((hipStream_t)stream, a);
}

cogs_status cogs_gemv_fp8(cogs_stream stream, const cogs_gemv_fp8_desc* d) {
    if (!d || !d->x || !d->W || !d->scale || !d->C) return COGS_E_INVALID;
    CogsGemm g;
    g.dtype = d->dtype;
    g.A = d->x; g.lda = d->K; g.W = d->W; g.ldw = d->ldw; g.C = d->C; g.ldc = d->N;
    g.bias = d->bias; g.residual = d->residual; g.ldr = d->N;
    g.M = 1; g.N = d->N; g.K = d->K; g.act = d->act; g.out_f32 = d->out_f32;
    g.rope_cos = d->rope_cos; g.rope_sin = d->rope_sin; g.rope_cols = d->rope_cols; g.head_dim = d->head_dim;
    if (d->q_scale != 0.f) { g.q_scale = d->q_scale; g.q_cols = d->q_cols; }
    g.rms_gamma = d->rms_gamma; g.rms_eps = d->rms_eps;
    g.kv_k = d->kv_k; g.kv_v = d->kv_v; g.kv_col0 = d->kv_col0; g.kv_dim = d->kv_dim;
    return cogs_k_gemv_fp8((hipStream_t)stream, g, d->scale);
}

cogs_status cogs_quantize_fp8_rows(cogs_stream stream, int dtype, const void* w, int64_t ldw, int N, int K, uint8_t* codes,
                                   int64_t ldq, float* scale, void* dequant, int64_t ldd) {
    return cogs_k_quantize_fp8_rows((hipStream_t)stream, dtype, w, ldw, N, K, codes, ldq, scale, dequant, ldd);
}

cogs_status cogs_ln_finalize(cogs_stream stream, const float* row_stats, int rows, int H, float eps, float* ln_ab) {
    if (!row_stats || !ln_ab || rows <= 0 || H <= 0 || H % 64) return COGS_E_INVALID;
    return cogs_k_ln_finalize((hipStream_t)stream, row_stats, rows, H / 64, H, eps, ln_ab);
}

cogs_status cogs_attention(cogs_stream stream, const cogs_attn_desc* d) {
    if (!d || !d->Q || !d->K || !d->V || !d->O) return COGS_E_INVALID;
    CogsAttn a;
    a.dtype = d->dtype; a.Q = d->Q; a.K = d->K; a.V = d->V; a.O = d->O;
    a.ldq = d->ldq; a.ldk = d->ldk; a.ldv = d->ldv; a.ldo = d->ldo;
    a.cu_seqlens = d->cu_seqlens; a.nseg = d->nseg; a.max_seqlen = d->max_seqlen;
    a.row_lo = d->row_lo; a.row_hi = d->row_hi; a.bias = d->bias;
    a.q_len = d->q_len; a.kv_len = d->kv_len; a.hq = d->hq; a.hkv = d->hkv; a.head_dim = d->head_dim;
    a.scale = d->scale; a.causal = d->causal; a.q_pos0 = d->q_pos0; a.force_rowwise = d->force_rowwise;
    a.nsplit = d->nsplit > 1 ? d->nsplit : 1; a.ws = d->ws; a.ws_bytes = d->ws_bytes;
    a.q_prescaled = d->q_prescaled;
    a.head_stride = d->head_stride;
    a.uniform_seqlen = (int)g_cogs_debug.attn_uniform_hint;      // 0 unless a test sets it (checked against q_len / max_seqlen by the kernel's launcher)
    return cogs_k_attention((hipStream_t)stream, a);
}

cogs_status cogs_layernorm(cogs_stream stream, int dtype, const void* x, void* y, const void* gamma, const void* beta,
                           int rows, int H, float eps) {
    return cogs_k_layernorm((hipStream_t)stream, dtype, x, y, gamma, beta, rows, H, eps);
}
cogs_status cogs_rmsnorm(cogs_stream stream, int dtype, const void* x, void* y, const void* gamma, int rows, int H,
                         float eps) {
    return cogs_k_rmsnorm((hipStream_t)stream, dtype, x, y, gamma, rows, H, eps);
}
cogs_status cogs_ln_merge(cogs_stream stream, int dtype, const void* x, void* y, const void* gamma, const void* beta,
                          int out_rows, int group, int H, float eps) {
    return cogs_k_ln_merge((hipStream_t)stream, dtype, x, y, gamma, beta, out_rows, group, H, eps);
}

cogs_status cogs_pixdiff_mask(cogs_stream stream, int dtype, const void* pix, int t, int P, int E, float thr,
                              int min_tokens, const uint8_t* minor, uint8_t* mask) {
    if (!pix || !mask) return COGS_E_INVALID;
    COGS_TRY(cogs_k_pixdiff_mask((hipStream_t)stream, dtype, pix, t, P, E, thr, min_tokens, mask));
    return cogs_k_mask_fix((hipStream_t)stream, mask, t, P, min_tokens, minor);
}
cogs_status cogs_frame_mean_to_slot0(cogs_stream stream, int dtype, void* feats, int P, int D, const int32_t* frames,
                                     int n_frames) {
    return cogs_k_frame_mean_to_slot0((hipStream_t)stream, dtype, feats, P, D, frames, n_frames);
}
cogs_status cogs_gather_rows(cogs_stream stream, int dtype, const void* ta, const void* tb, const int64_t* idx,
                             void* out, int rows, int D) {
    return cogs_k_gather_rows((hipStream_t)stream, dtype, ta, tb, idx, out, rows, D);
}
cogs_status cogs_mean_rows(cogs_stream stream, int dtype, const void* x, int64_t ldx, int rows, int D, float* out) {
    return cogs_k_mean_rows((hipStream_t)stream, dtype, x, ldx, rows, D, out);
}
cogs_status cogs_cosine(cogs_stream stream, const float* a, const float* b, int n, int D, float* out) {
    return cogs_k_cosine((hipStream_t)stream, a, b, n, D, out);
}

cogs_status cogs_kmeans_workspace_bytes(int T, int64_t PD, int K, size_t* bytes) {
    if (!bytes || T <= 0 || PD <= 0 || K <= 0) return COGS_E_INVALID;
    *bytes = align_up(cogs_k_kmeans_ws(T, PD, K, nullptr));
    return COGS_OK;
}
cogs_status cogs_kmeans_sqdist(cogs_stream stream, int dtype, const void* feats, int T, int64_t PD,
                               const float* centres, const int32_t* centre_rows, int K, float* dist2, void* ws,
                               size_t ws_bytes) {
    int ns = 0;
    const size_t need = cogs_k_kmeans_ws(T, PD, K, &ns);
    if (!ws || ws_bytes < need) return COGS_E_WORKSPACE;
    if (!centres && !centre_rows) return COGS_E_INVALID;
    return cogs_k_kmeans_sqdist((hipStream_t)stream, dtype, feats, T, PD, centres, centre_rows, K, (float*)ws, ns, dist2);
}
cogs_status cogs_kmeans_assign(cogs_stream stream, const float* dist2, const float* ts, const float* centre_ts, int T,
                               int K, float alpha, int64_t* assign, int32_t* counts) {
    return cogs_k_kmeans_assign((hipStream_t)stream, dist2, ts, centre_ts, T, K, alpha, assign, counts);
}
cogs_status cogs_kmeans_update(cogs_stream stream, int dtype, const void* feats, const float* ts, int T, int64_t PD,
                               int K, const int64_t* assign, const int32_t* reseed_rows, float* centres,
                               float* centre_ts, float* shift_out, void* ws, size_t ws_bytes) {
    const size_t need = cogs_k_kmeans_ws(T, PD, K, nullptr);
    if (!ws || ws_bytes < need) return COGS_E_WORKSPACE;
    return cogs_k_kmeans_update((hipStream_t)stream, dtype, feats, ts, T, PD, K, assign, reseed_rows, centres,
                                centre_ts, (float*)ws, cogs_k_kmeans_update_blocks(PD), shift_out);
}
cogs_status cogs_select_near_centroid(cogs_stream stream, const float* dist2, const int64_t* assign, int T, int K, int n_extra,
                                      int64_t* out_idx, int32_t* out_counts) {
    if (!dist2 || !assign || !out_idx || !out_counts) return COGS_E_INVALID;
    return cogs_k_select_near((hipStream_t)stream, dist2, assign, T, K, n_extra, out_idx, out_counts);
}
cogs_status cogs_kmeans_pp_step(cogs_stream stream, int dtype, const void* feats, int T, int64_t PD, int row, int first,
                                float* nearest2, float* probs_host, void* ws, size_t ws_bytes) {
    int ns = 0;
    const size_t need = cogs_k_kmeans_ws(T, PD, 1, &ns);
    if (!ws || ws_bytes < need) return COGS_E_WORKSPACE;
    if (!feats || !nearest2 || T <= 0) return COGS_E_INVALID;
    return cogs_k_kmeans_pp_step((hipStream_t)stream, dtype, feats, T, PD, row, first, nearest2, probs_host, (float*)ws, ns);
}
cogs_status cogs_kmeans_pp(cogs_stream stream, int dtype, const void* feats, int T, int64_t PD, int K, int first_row,
                           const float* q_draws, int32_t* idx, int32_t* zero_flag, float* nearest2, void* ws, size_t ws_bytes) {
    int ns = 0;
    const size_t need = cogs_k_kmeans_ws(T, PD, 1, &ns);
    if (!ws || ws_bytes < need) return COGS_E_WORKSPACE;
    if (!feats || !q_draws || !idx || !zero_flag || !nearest2 || T <= 0 || K <= 0) return COGS_E_INVALID;
    return cogs_k_kmeans_pp((hipStream_t)stream, dtype, feats, T, PD, K, first_row, q_draws, idx, zero_flag, nearest2, (float*)ws, ns);
}
cogs_status cogs_kmeans_margins(cogs_stream stream, int T, int64_t PD, int K, void* ws, size_t ws_bytes, float* min_margin,
                                int32_t* rows_below) {
    const size_t need = cogs_k_kmeans_ws(T, PD, K, nullptr);
    if (!ws || ws_bytes < need) return COGS_E_WORKSPACE;
    return cogs_k_kmeans_margins((hipStream_t)stream, T, PD, K, (float*)ws, min_margin, rows_below);
}
cogs_status cogs_kmeans_lloyd(cogs_stream stream, int dtype, const void* feats, const float* ts, int T, int64_t PD, int K,
                              float alpha, int max_iter, float tol, const int32_t* reseed_pool, int pool_len,
                              float* centres, float* centre_ts, int64_t* assign, int* iterations, int* reseeds_used,
                              int* pool_exhausted, void* ws, size_t ws_bytes) {
    int ns = 0;
    const size_t need = cogs_k_kmeans_ws(T, PD, K, &ns);
    if (!ws || ws_bytes < need) return COGS_E_WORKSPACE;
    if (!feats || !ts || !centres || !centre_ts || !assign || (pool_len > 0 && !reseed_pool)) return COGS_E_INVALID;
    return cogs_k_kmeans_lloyd((hipStream_t)stream, dtype, feats, ts, T, PD, K, alpha, max_iter, tol, reseed_pool, pool_len,
                               centres, centre_ts, assign, iterations, reseeds_used, pool_exhausted, (float*)ws, ns);
}
cogs_status cogs_pack_rows(cogs_stream stream, int in_dtype, int out_dtype, const void* in, int64_t ld_in, void* out,
                           int64_t ld_out, int rows, int cols_in, int cols_out) {
    return cogs_k_pack_rows((hipStream_t)stream, in_dtype, out_dtype, in, ld_in, out, ld_out, rows, cols_in, cols_out);
}

cogs_status cogs_preprocess_workspace_bytes(int T, int H, int tw, size_t* bytes) {
    if (!bytes || T <= 0 || H <= 0 || tw <= 0) return COGS_E_INVALID;
    *bytes = align_up((size_t)T * H * tw * 3);
    return COGS_OK;
}
cogs_status cogs_preprocess_frames(cogs_stream stream, const uint8_t* frames, int T, int H, int W, int th, int tw,
                                   int merge, const int32_t* bounds_x, const int32_t* coef_x, int ksx,
                                   const int32_t* bounds_y, const int32_t* coef_y, int ksy, const float* value_table,
                                   void* out, int out_dtype, void* ws, size_t ws_bytes) {
    if (!frames || !out || !bounds_x || !coef_x || !bounds_y || !coef_y || !value_table) return COGS_E_INVALID;
    if (!ws || ws_bytes < (size_t)T * H * tw * 3) return COGS_E_WORKSPACE;
    return cogs_k_preprocess((hipStream_t)stream, frames, T, H, W, th, tw, merge, bounds_x, coef_x, ksx, bounds_y,
                             coef_y, ksy, out, out_dtype, value_table, (uint8_t*)ws);
}

cogs_status cogs_argmax(cogs_stream stream, const float* logits, int n, int64_t* out, void* ws) {
    if (!ws) return COGS_E_WORKSPACE;
    return cogs_k_argmax((hipStream_t)stream, logits, n, out, (float*)ws);
}
cogs_status cogs_logits_process(cogs_stream stream, float* logits, int n, const int64_t* prev, int n_prev,
                                float repetition_penalty, const int32_t* allowed, int n_allowed, float temperature,
                                float* tmp) {
    if (n_prev > 0 && !tmp) return COGS_E_WORKSPACE;
    return cogs_k_logits_process((hipStream_t)stream, logits, n, prev, n_prev, repetition_penalty, allowed, n_allowed,
                                 temperature, tmp);
}

cogs_status cogs_row_lse_workspace_bytes(int rows, int n, size_t* bytes) {
    if (rows <= 0 || n <= 0 || !bytes) return COGS_E_INVALID;
    CogsLsePlan p; cogs_k_lse_plan(rows, n, &p);
    *bytes = lse_scratch(p, false, nullptr).bytes;
    return COGS_OK;
}
cogs_status cogs_row_lse(cogs_stream stream, const float* logits, int rows, int n, int64_t ld, const int64_t* targets,
                         float* lse, float* target_logit, int64_t* argmax, float* max_logit, int32_t* n_bad, void* ws,
                         size_t ws_bytes) {
    if (!logits || rows <= 0 || n <= 0 || (n & 3) || ld < n || (ld & 3) || ((uintptr_t)logits & 15)) return COGS_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    CogsLsePlan p; cogs_k_lse_plan(rows, n, &p);
    const LseScratch b = lse_scratch(p, false, ws);
    if (!ws || ws_bytes < b.bytes) return COGS_E_WORKSPACE;
    lse_report(p);
    for (int r0 = 0; r0 < rows; r0 += p.rows_b) {
        const int rb = rows - r0 < p.rows_b ? rows - r0 : p.rows_b;
        for (int c0 = 0; c0 < n; c0 += p.cols_p) {
            const int wd = n - c0 < p.cols_p ? n - c0 : p.cols_p;
            COGS_TRY(cogs_k_lse_fold(st, p, logits + (size_t)r0 * ld + c0, ld, rb, wd, c0, targets ? targets + r0 : nullptr,
                                     target_logit ? target_logit + r0 : nullptr, (char*)b.state + (size_t)r0 * 16, b.part));
        }
    }
    return cogs_k_lse_final(st, b.state, rows, n, targets, lse, target_logit, argmax, max_logit, n_bad);
}

size_t cogs_sample_workspace_bytes(void) { return cogs_k_sample_ws(); }
cogs_status cogs_sample(cogs_stream stream, const float* logits, int n, float temperature, int top_k, double top_p,
                        const float* draws,
                        uint64_t seed, uint64_t offset, int64_t* out_token, int32_t* kept_idx, float* kept_prob,
                        int32_t* n_kept, int kept_cap, void* ws) {
    return cogs_k_sample((hipStream_t)stream, logits, n, temperature, top_k, top_p, draws, seed, offset, out_token, kept_idx, kept_prob,
                         n_kept, kept_cap, ws);
}
cogs_status cogs_topk(cogs_stream stream, const float* logits, int n, int top_k, float* topk_val, int32_t* topk_idx,
                      float* ws) {
    if (!ws) return COGS_E_WORKSPACE;
    return cogs_k_topk((hipStream_t)stream, logits, n, top_k, topk_val, topk_idx, ws);
}

cogs_status cogs_beam_topk_workspace_bytes(int rows, int n, int k, size_t* bytes) {
    if (!bytes) return COGS_E_INVALID;
    return cogs_k_beam_topk_ws(rows, n, k, bytes);
}
cogs_status cogs_beam_topk(cogs_stream stream, const float* scores, int rows, int n, int64_t ld, const float* row_add, int k,
                           float* out_val, int32_t* out_row, int32_t* out_tok, void* ws, size_t ws_bytes) {
    return cogs_k_beam_topk((hipStream_t)stream, scores, rows, n, ld, row_add, k, out_val, out_row, out_tok, ws, ws_bytes);
}
cogs_status cogs_sub_rows(cogs_stream stream, float* x, int rows, int n, int64_t ld, const float* sub) {
    return cogs_k_sub_rows((hipStream_t)stream, x, rows, n, ld, sub);
}

}  // extern "C"
