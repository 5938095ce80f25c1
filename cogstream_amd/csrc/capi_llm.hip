// C-ABI layer, language-model side: Qwen2 weights, the forward over a prompt / one token / several segments, the lockstep
// multi-row decode step and teacher-forced scoring. Handle, carver and profiling bracket: capi_internal.h.
#include "capi_internal.h"

// workspace of a forward over S rows, or of a lockstep step over R rows (base == nullptr: only `bytes` is meaningful)
struct LlmScratch {
    void *x, *ln, *qkv, *att, *act;      // residual stream, RMSNorm(x), [q | k | v], attention output, MLP hidden
    float* rc;                           // interleaved (cos, sin) table
    void* split; size_t split_bytes;     // decode-attention partials
    int32_t *pos, *cu;                   // per-row positions; cu_seqlens (forward only)
    size_t bytes;
};
static void llm_scratch_rows(const cogs_llm_weights& w, int M, Carver& c, LlmScratch& s) {      // the part both layouts start with
    const size_t es = esize(w.dtype);
    const int qd = (w.heads + 2 * w.kv_heads) * w.head_dim;
    s.x = c.take((size_t)M * w.hidden * es);
    s.ln = c.take((size_t)M * w.hidden * es);
    s.qkv = c.take((size_t)M * qd * es);
    s.att = c.take((size_t)M * w.heads * w.head_dim * es);
    s.act = c.take((size_t)M * w.inter * es);
    s.rc = (float*)c.take((size_t)M * (w.head_dim / 2) * 2 * sizeof(float));
}
// (split counts and partial-buffer sizes: attn_plan.h, under the switches `t` the caller snapshot once)
static LlmScratch llm_scratch(const cogs_llm_weights& w, int S, int max_ctx, const AttnTuning& t, void* base) {
    Carver c(base);
    LlmScratch s{};
    llm_scratch_rows(w, S, c, s);
    s.split_bytes = cogs_attn_split_ws_bytes(cogs_attn_nsplit(max_ctx, t), 1, w.heads, w.head_dim);
    s.split = c.take(s.split_bytes);
    s.pos = (int32_t*)c.take((size_t)S * sizeof(int32_t));          // per-row positions (segmented forward)
    s.cu = (int32_t*)c.take(((size_t)S + 1) * sizeof(int32_t));     // cu_seqlens (at most S segments)
    s.bytes = c.off;
    return s;
}
static LlmScratch rows_scratch(const cogs_llm_weights& w, int R, int max_prefix, const AttnTuning& t, void* base) {
    Carver c(base);
    LlmScratch s{};
    llm_scratch_rows(w, R, c, s);
    s.pos = (int32_t*)c.take((size_t)R * sizeof(int32_t));
    s.split_bytes = cogs_attn_split_ws_bytes(cogs_attn_rows_nsplit(max_prefix, t) + 1, R, w.heads, w.head_dim);
    s.split = c.take(s.split_bytes);
    s.bytes = c.off;
    return s;
}

// row `row` of layer l in a [layers][max_len][kv_dim] cache
static char* kv_row(void* base, int l, int max_len, int row, size_t row_bytes) {
    return (char*)base + ((size_t)l * max_len + row) * row_bytes;
}

// ---- one decoder layer, written once. Its callers differ in LayerArgs and in two callables:
//   linear(g, codes, scales)   launches the GEMM of one linear: cogs_k_gemm, the e4m3 GEMV on (codes, scales), cogs_k_gemm_rows, or
//                              cogs_k_gemm_rows_fp8 on (codes, scales)
//   attend(l)                  everything between the QKV GEMM and the out-projection: puts the new K / V rows where they
//                              belong and runs the attention from b.qkv into b.att
struct LayerArgs {
    int M;                      // rows
    const void* xin;            // the residual stream entering the layer: b.x, or the embedding row read in place
    bool fuse_norm;             // RMSNorm runs inside the GEMV prologue (single-token decode) instead of as its own kernel
    bool prescale_q;            // Q leaves the QKV GEMM multiplied by scale * log2(e) (see VitRange::begin)
    void *kv_k, *kv_v;          // the QKV GEMV writes the new K / V row here (null: attend() places the rows)
    cogs_llm_fp8_layer F;       // the layer's e4m3 codes and scales for linear() (all null: the weights' own type)
};

template <class Linear, class Attend>
static cogs_status llm_layer(cogs_handle h, hipStream_t st, int l, const LlmScratch& b, const LayerArgs& a, Linear linear,
                             Attend attend) {
    const cogs_llm_weights& w = h->llm;
    const cogs_llm_layer& L = h->llm_layers[l];
    const int dt = w.dtype, M = a.M;
    const int H = w.hidden, hd = w.head_dim, kvd = w.kv_heads * hd, qd_q = w.heads * hd, qd = qd_q + 2 * kvd;
    if (!a.fuse_norm) { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_rmsnorm(st, dt, b.x, b.ln, L.in_ln, M, H, w.rms_eps)); }
    {
        CogsGemm g; g.dtype = dt;
        g.A = a.fuse_norm ? a.xin : b.ln; g.lda = H; g.W = L.qkv_w; g.ldw = H; g.C = b.qkv; g.ldc = qd;
        g.bias = L.qkv_b; g.M = M; g.N = qd; g.K = H;
        g.rope_cos = b.rc; g.rope_sin = nullptr; g.rope_cols = qd_q + kvd; g.head_dim = hd;
        if (a.prescale_q) { g.q_scale = 1.0f / sqrtf((float)hd) * 1.4426950408889634f; g.q_cols = qd_q; }
        if (a.fuse_norm) { g.rms_gamma = L.in_ln; g.rms_eps = w.rms_eps; }
        if (a.kv_k) { g.kv_k = a.kv_k; g.kv_v = a.kv_v; g.kv_col0 = qd_q; g.kv_dim = kvd; }
        { PROF(COGS_PROF_GEMM); COGS_TRY(linear(g, a.F.qkv_q, a.F.qkv_s)); }
    }
    COGS_TRY(attend(l));
    {
        CogsGemm g; g.dtype = dt;
        g.A = b.att; g.lda = qd_q; g.W = L.o_w; g.ldw = qd_q; g.C = b.x; g.ldc = H;
        g.residual = a.xin; g.ldr = H; g.M = M; g.N = H; g.K = qd_q;
        { PROF(COGS_PROF_GEMM); COGS_TRY(linear(g, a.F.o_q, a.F.o_s)); }
    }
    if (!a.fuse_norm) { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_rmsnorm(st, dt, b.x, b.ln, L.post_ln, M, H, w.rms_eps)); }
    {
        CogsGemm g; g.dtype = dt;
        g.A = a.fuse_norm ? b.x : b.ln; g.lda = H; g.W = L.gu_w; g.ldw = H; g.C = b.act; g.ldc = w.inter;
        g.M = M; g.N = 2 * w.inter; g.K = H; g.act = COGS_ACT_SWIGLU;
        if (a.fuse_norm) { g.rms_gamma = L.post_ln; g.rms_eps = w.rms_eps; }
        { PROF(COGS_PROF_GEMM); COGS_TRY(linear(g, a.F.gu_q, a.F.gu_s)); }
    }
    {
        CogsGemm g; g.dtype = dt;
        g.A = b.act; g.lda = w.inter; g.W = L.down_w; g.ldw = w.inter; g.C = b.x; g.ldc = H;
        g.residual = b.x; g.ldr = H; g.M = M; g.N = H; g.K = w.inter;
        { PROF(COGS_PROF_GEMM); COGS_TRY(linear(g, a.F.down_q, a.F.down_s)); }
    }
    return COGS_OK;
}

// lm_head on M rows of final-norm hidden states at A -> fp32 C: vocabulary columns [col0, col0 + cols)
static CogsGemm lm_head_gemm(const cogs_llm_weights& w, const void* A, int M, float* C, long ldc, int col0, int cols) {
    CogsGemm g; g.dtype = w.dtype;
    g.A = A; g.lda = w.hidden; g.W = (const char*)w.lm_head + (size_t)col0 * w.hidden * esize(w.dtype); g.ldw = w.hidden;
    g.C = C; g.ldc = ldc; g.M = M; g.N = cols; g.K = w.hidden; g.out_f32 = 1;
    return g;
}

// one implementation behind cogs_llm_forward and cogs_llm_forward_segments: nseg > 0 = stateless forward over
// nseg independent sequences stored back to back (causal attention and positions restart at every cu_host[s])
static cogs_status llm_forward_impl(cogs_handle h, cogs_stream stream, const void* embeds, int S, cogs_kv* kv,
                                    float* last_logits, float* pooled_mean, void* hidden_out, void* ws, size_t ws_bytes,
                                    const int32_t* cu_host, int nseg, float* pooled_seg) {
    if (!h || !h->llm_ok || !embeds || S <= 0) return COGS_E_INVALID;
    const cogs_llm_weights& w = h->llm;
    hipStream_t st = (hipStream_t)stream;
    const int dt = w.dtype;
    const size_t es = esize(dt);
    const int H = w.hidden, hd = w.head_dim, kvd = w.kv_heads * hd, qd_q = w.heads * hd, qd = qd_q + 2 * kvd;
    const int pos0 = kv ? kv->len : 0;
    const int ctx = pos0 + S;
    if (kv && (!kv->k || !kv->v || ctx > kv->max_len)) return COGS_E_INVALID;
    const AttnTuning tune = cogs_k_attention_tuning();
    const LlmScratch b = llm_scratch(w, S, ctx, tune, ws);
    if (!ws || ws_bytes < b.bytes) return COGS_E_WORKSPACE;
    int max_seg = 0;
    if (nseg > 0) {
        if (kv || !cu_host || cu_host[0] != 0 || cu_host[nseg] != S || nseg > S) return COGS_E_INVALID;
        for (int sgm = 0; sgm < nseg; ++sgm) {
            const int lo = cu_host[sgm], hi = cu_host[sgm + 1];
            if (hi <= lo) return COGS_E_INVALID;
            max_seg = hi - lo > max_seg ? hi - lo : max_seg;
        }
        // segment boundaries through the pinned ring (the caller's array may die when this call returns);
        // per-row positions from them on the device
        COGS_TRY(stage_h2d(h, st, b.cu, cu_host, (size_t)(nseg + 1) * sizeof(int32_t)));
        { PROF(COGS_PROF_OTHER); COGS_TRY(cogs_k_seg_positions(st, b.cu, nseg, b.pos)); }
    }

    // single-token decode reads the new embedding row in place (layer 0's qkv input and residual source), everything
    // else copies the prompt rows into the residual stream first
    const bool embeds_in_place = (S == 1 && nseg == 0);
    if (!embeds_in_place && hipMemcpyAsync(b.x, embeds, (size_t)S * H * es, hipMemcpyDeviceToDevice, st) != hipSuccess) return COGS_E_HIP;
    { PROF(COGS_PROF_OTHER); COGS_TRY(cogs_k_llm_rope_table(st, b.rc, nullptr, nseg > 0 ? b.pos : nullptr, pos0, S, h->llm_inv_freq, hd / 2)); }
    const bool prescale_q = dt == COGS_DT_BF16 && hd == 128;   // see VitRange::begin
    // single-token steps read the attached e4m3 codes (cogs_llm_attach_fp8); every other row count, and the lm_head GEMV
    // behind a prompt, reads the (dequantised) matrices of cogs_llm_weights: prefill results do not depend on the mode
    const bool fp8 = S == 1 && h->fp8_ok && g_cogs_debug.llm_decode_fp8 != 0;
    g_cogs_debug.llm_last_decode_fp8 = fp8 ? 1 : 0;
    auto linear = [&](CogsGemm& g, const uint8_t* codes, const float* scales) -> int {
        if (!fp8) return cogs_k_gemm(st, g);
        g.W = codes; g.ldw = g.K;
        return cogs_k_gemv_fp8(st, g, scales);
    };
    // K / V: with a cache, the attention reads the cache rows (a prompt's rows are appended first; a single token's row is
    // already there, written by the QKV GEMV); without one, the qkv buffer itself
    auto attend = [&](int l) -> int {
        const char* kp = (const char*)b.qkv + (size_t)qd_q * es;
        const char* vp = kp + (size_t)kvd * es;
        long ldkv = qd;
        if (kv) {
            if (S != 1) {
                PROF(COGS_PROF_OTHER);
                COGS_TRY(cogs_k_kv_append(st, dt, kp, vp, qd, kv_row(kv->k, l, kv->max_len, pos0, kvd * es),
                                          kv_row(kv->v, l, kv->max_len, pos0, kvd * es), kvd, S, kvd));
            }
            kp = kv_row(kv->k, l, kv->max_len, 0, kvd * es); vp = kv_row(kv->v, l, kv->max_len, 0, kvd * es); ldkv = kvd;
        }
        CogsAttn a; a.dtype = dt;
        a.Q = b.qkv; a.K = kp; a.V = vp; a.O = b.att;
        a.ldq = qd; a.ldk = ldkv; a.ldv = ldkv; a.ldo = qd_q;
        a.q_len = S; a.kv_len = ctx; a.hq = w.heads; a.hkv = w.kv_heads; a.head_dim = hd; a.scale = 1.0f / sqrtf((float)hd);
        a.causal = 1; a.q_pos0 = pos0; a.q_prescaled = prescale_q;
        if (nseg > 0) { a.cu_seqlens = b.cu; a.nseg = nseg; a.max_seqlen = max_seg; }
        if (S == 1 && dt == COGS_DT_BF16 && hd == 128) { a.nsplit = cogs_attn_nsplit(ctx, tune); a.ws = b.split; a.ws_bytes = b.split_bytes; }
        PROF(COGS_PROF_ATTN);
        return cogs_k_attention(st, a);
    };
    for (int l = 0; l < w.layers; ++l) {
        const bool kv_fused = kv && S == 1;     // single-token decode: the GEMV writes the new K / V row straight into the cache
        const LayerArgs a{S, (embeds_in_place && l == 0) ? embeds : (const void*)b.x, S == 1, prescale_q,
                          kv_fused ? kv_row(kv->k, l, kv->max_len, pos0, kvd * es) : nullptr,
                          kv_fused ? kv_row(kv->v, l, kv->max_len, pos0, kvd * es) : nullptr,
                          fp8 ? h->fp8_layers[l] : cogs_llm_fp8_layer{}};
        COGS_TRY(llm_layer(h, st, l, b, a, linear, attend));
    }
    if (kv) kv->len = ctx;
    if (nseg > 0) {   // final norm over every row, then one mean per sequence
        if (!pooled_seg) return COGS_E_INVALID;
        { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_rmsnorm(st, dt, b.x, b.ln, w.final_norm, S, H, w.rms_eps)); }
        for (int sgm = 0; sgm < nseg; ++sgm) {
            PROF(COGS_PROF_OTHER);
            COGS_TRY(cogs_k_mean_rows(st, dt, (const char*)b.ln + (size_t)cu_host[sgm] * H * es, H,
                                      cu_host[sgm + 1] - cu_host[sgm], H, pooled_seg + (size_t)sgm * H));
        }
        return COGS_OK;
    }
    const void* last = b.x;     // where the lm_head reads the last row from
    const bool need_all = pooled_mean || hidden_out;
    if (need_all) {
        void* hn = hidden_out ? hidden_out : b.ln;
        { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_rmsnorm(st, dt, b.x, hn, w.final_norm, S, H, w.rms_eps)); }
        if (pooled_mean) { PROF(COGS_PROF_OTHER); COGS_TRY(cogs_k_mean_rows(st, dt, hn, H, S, H, pooled_mean)); }
        last = hn;
    }
    if (last_logits) {
        CogsGemm g = lm_head_gemm(w, (const char*)last + (size_t)(S - 1) * H * es, 1, last_logits, w.vocab, 0, w.vocab);
        if (!need_all) { g.rms_gamma = w.final_norm; g.rms_eps = w.rms_eps; }   // final RMSNorm fused into the lm_head GEMV
        { PROF(COGS_PROF_GEMM); COGS_TRY(linear(g, h->fp8.lm_head_q, h->fp8.lm_head_s)); }
    }
    return COGS_OK;
}

extern "C" {

cogs_status cogs_llm_load(cogs_handle h, const cogs_llm_weights* w) {
    if (!h || !w || !w->layer || w->layers <= 0) return COGS_E_INVALID;
    if (w->heads % w->kv_heads || w->head_dim % 8 || w->vocab % 4) return COGS_E_INVALID;
    const int slab = w->dtype == COGS_DT_BF16 ? 64 : 32;
    if (w->hidden % slab || w->inter % slab || (w->heads * w->head_dim) % slab) return COGS_E_INVALID;
    h->llm = *w;
    h->fp8_ok = false;      // the codes of cogs_llm_attach_fp8 belong to the weight set they were made from
    h->llm_layers.assign(w->layer, w->layer + w->layers);
    h->llm.layer = h->llm_layers.data();
    // Qwen2RotaryEmbedding: inv_freq = 1 / theta^(arange(0, hd, 2)/hd)
    const int nf = w->head_dim / 2;
    std::vector<float> inv(nf);
    for (int i = 0; i < nf; ++i) inv[i] = 1.0f / powf(w->rope_theta, (float)(2 * i) / (float)w->head_dim);
    // re-pointing the handle at another weight set of the same shape (adapter switch) keeps the device table
    if (!h->llm_inv_freq || h->llm_nfreq != nf || h->llm_theta != w->rope_theta) {
        if (h->llm_inv_freq) (void)hipFree(h->llm_inv_freq);
        h->llm_inv_freq = nullptr;
        if (hipMalloc(&h->llm_inv_freq, nf * sizeof(float)) != hipSuccess) return COGS_E_HIP;
        if (hipMemcpy(h->llm_inv_freq, inv.data(), nf * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return COGS_E_HIP;
        h->llm_nfreq = nf; h->llm_theta = w->rope_theta;
    }
    h->llm_ok = true;
    return COGS_OK;
}

cogs_status cogs_llm_attach_fp8(cogs_handle h, const cogs_llm_fp8_weights* w) {
    if (!h) return COGS_E_INVALID;
    if (!w) { h->fp8_ok = false; return COGS_OK; }
    if (!h->llm_ok || !w->layer || w->layers != h->llm.layers || !w->lm_head_q || !w->lm_head_s) return COGS_E_INVALID;
    const cogs_llm_weights& m = h->llm;
    if (m.hidden % 16 || m.inter % 16 || (m.heads * m.head_dim) % 16) return COGS_E_INVALID;
    for (int l = 0; l < w->layers; ++l) {
        const cogs_llm_fp8_layer& L = w->layer[l];
        if (!L.qkv_q || !L.o_q || !L.gu_q || !L.down_q || !L.qkv_s || !L.o_s || !L.gu_s || !L.down_s) return COGS_E_INVALID;
    }
    h->fp8 = *w;
    h->fp8_layers.assign(w->layer, w->layer + w->layers);
    h->fp8.layer = h->fp8_layers.data();
    h->fp8_ok = true;
    return COGS_OK;
}

cogs_status cogs_llm_workspace_bytes(cogs_handle h, int max_tokens, int max_context, size_t* bytes) {
    if (!h || !h->llm_ok || !bytes || max_tokens <= 0) return COGS_E_INVALID;
    *bytes = llm_scratch(h->llm, max_tokens, max_context, cogs_k_attention_tuning(), nullptr).bytes;
    return COGS_OK;
}

cogs_status cogs_llm_decode_rows_workspace_bytes(cogs_handle h, int R, int max_prefix, size_t* bytes) {
    if (!h || !h->llm_ok || !bytes || R <= 0 || max_prefix <= 0) return COGS_E_INVALID;
    *bytes = rows_scratch(h->llm, R, max_prefix, cogs_k_attention_tuning(), nullptr).bytes;
    return COGS_OK;
}

cogs_status cogs_llm_forward(cogs_handle h, cogs_stream stream, const void* embeds, int S, cogs_kv* kv,
                             float* last_logits, float* pooled_mean, void* hidden_out, void* ws, size_t ws_bytes) {
    return llm_forward_impl(h, stream, embeds, S, kv, last_logits, pooled_mean, hidden_out, ws, ws_bytes, nullptr, 0, nullptr);
}

cogs_status cogs_llm_forward_segments(cogs_handle h, cogs_stream stream, const void* embeds, int S,
                                      const int32_t* cu_seqlens_host, int nseg, float* pooled_means, void* ws,
                                      size_t ws_bytes) {
    if (nseg <= 0 || !cu_seqlens_host || !pooled_means) return COGS_E_INVALID;
    return llm_forward_impl(h, stream, embeds, S, nullptr, nullptr, nullptr, nullptr, ws, ws_bytes, cu_seqlens_host, nseg,
                            pooled_means);
}

// ---- teacher-forced scoring

cogs_status cogs_lm_score_workspace_bytes(cogs_handle h, int S, size_t* bytes) {
    if (!h || !h->llm_ok || !bytes || S <= 0) return COGS_E_INVALID;
    CogsLsePlan p; cogs_k_lse_plan(S, h->llm.vocab, &p);
    *bytes = lse_scratch(p, true, nullptr).bytes;
    return COGS_OK;
}

// row blocks x vocabulary panels: lm_head GEMM with fp32 output into the panel (the accumulators last_logits comes from),
// fold into the per-row state, next panel; one last kernel for the outputs. Everything on the caller's stream.
cogs_status cogs_lm_score(cogs_handle h, cogs_stream stream, const void* hidden, int S, const int64_t* targets, float* lse,
                          float* target_logit, int64_t* argmax, float* max_logit, int32_t* n_bad, void* ws,
                          size_t ws_bytes) {
    if (!h || !h->llm_ok || !hidden || S <= 0) return COGS_E_INVALID;
    const cogs_llm_weights& w = h->llm;
    hipStream_t st = (hipStream_t)stream;
    const size_t es = esize(w.dtype);
    const int H = w.hidden, V = w.vocab;
    CogsLsePlan p; cogs_k_lse_plan(S, V, &p);
    const LseScratch b = lse_scratch(p, true, ws);
    if (!ws || ws_bytes < b.bytes) return COGS_E_WORKSPACE;
    lse_report(p);
    for (int r0 = 0; r0 < S; r0 += p.rows_b) {
        const int rb = S - r0 < p.rows_b ? S - r0 : p.rows_b;
        for (int c0 = 0; c0 < V; c0 += p.cols_p) {
            const int wd = V - c0 < p.cols_p ? V - c0 : p.cols_p;
            CogsGemm g = lm_head_gemm(w, (const char*)hidden + (size_t)r0 * H * es, rb, b.panel, p.cols_p, c0, wd);
            { PROF(COGS_PROF_GEMM); COGS_TRY(cogs_k_gemm(st, g)); }
            { PROF(COGS_PROF_OTHER);
              COGS_TRY(cogs_k_lse_fold(st, p, b.panel, p.cols_p, rb, wd, c0, targets ? targets + r0 : nullptr,
                                       target_logit ? target_logit + r0 : nullptr, (char*)b.state + (size_t)r0 * 16, b.part)); }
        }
    }
    PROF(COGS_PROF_OTHER);
    return cogs_k_lse_final(st, b.state, S, V, targets, lse, target_logit, argmax, max_logit, n_bad);
}

// ---- lockstep decode of R continuations of one prompt

cogs_status cogs_llm_decode_rows(cogs_handle h, cogs_stream stream, const void* embeds, int R, cogs_kv_rows* kv, float* logits,
                                 void* ws, size_t ws_bytes) {
    return cogs_llm_decode_rows_slots(h, stream, embeds, R, kv, nullptr, logits, ws, ws_bytes);
}

// tail_slot [R][tail_max] (null: row r reads slot r): row r's new K / V still goes to slot r, position tail_len -- the caller has
// set tail_slot[r][tail_len] = r -- and the attention reads every row's tail through the table
cogs_status cogs_llm_decode_rows_slots(cogs_handle h, cogs_stream stream, const void* embeds, int R, cogs_kv_rows* kv,
                                       const int32_t* tail_slot, float* logits, void* ws, size_t ws_bytes) {
    if (!h || !h->llm_ok || !embeds || !kv || !logits || R <= 0) return COGS_E_INVALID;
    const cogs_llm_weights& w = h->llm;
    if (w.dtype != COGS_DT_BF16 || w.head_dim != 128 || R > 16) return COGS_E_UNSUPPORTED;
    if (!kv->k || !kv->v || !kv->tail_k || !kv->tail_v || kv->prefix_len < 1 || kv->prefix_len > kv->max_len || kv->tail_len < 0 ||
        kv->tail_len >= kv->tail_max)
        return COGS_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int dt = w.dtype;
    const size_t es = esize(dt);
    const int H = w.hidden, hd = w.head_dim, kvd = w.kv_heads * hd, qd_q = w.heads * hd, qd = qd_q + 2 * kvd;
    const AttnTuning tune = cogs_k_attention_tuning();
    const LlmScratch b = rows_scratch(w, R, kv->prefix_len, tune, ws);
    if (!ws || ws_bytes < b.bytes) return COGS_E_WORKSPACE;
    // llm_last_decode_fp8 speaks of single-token cogs_llm_forward steps only. With e4m3 codes attached and llm_rows_fp8 on, this
    // step streams the codes through cogs_k_gemm_rows_fp8, else the (dequantised) matrices of cogs_llm_weights: the same bits
    g_cogs_debug.llm_last_decode_fp8 = 0;
    const bool fp8 = h->fp8_ok && g_cogs_debug.llm_rows_fp8 != 0;
    g_cogs_debug.llm_last_rows_fp8 = fp8 ? 1 : 0;
    const int tl = kv->tail_len, position = kv->prefix_len + tl;      // lockstep: one position, one rotary row for every row
    if (hipMemcpyAsync(b.x, embeds, (size_t)R * H * es, hipMemcpyDeviceToDevice, st) != hipSuccess) return COGS_E_HIP;
    if (hipMemsetD32Async((hipDeviceptr_t)b.pos, position, R, st) != hipSuccess) return COGS_E_HIP;
    { PROF(COGS_PROF_OTHER); COGS_TRY(cogs_k_llm_rope_table(st, b.rc, nullptr, b.pos, 0, R, h->llm_inv_freq, hd / 2)); }
    const int nsplit = cogs_attn_rows_nsplit(kv->prefix_len, tune);
    const size_t tail_row = (size_t)kv->tail_max * kvd;               // elements between two rows' tails
    auto linear = [&](CogsGemm& g, const uint8_t* codes, const float* scales) -> int {
        if (!fp8) return cogs_k_gemm_rows(st, g);
        g.W = codes; g.ldw = g.K;
        return cogs_k_gemm_rows_fp8(st, g, scales);
    };
    // K / V: every row's new K / V goes behind its own tail; the attention reads the shared prefix and the row's tail
    auto attend = [&](int l) -> int {
        char* tk = (char*)kv->tail_k + (size_t)l * R * tail_row * es;
        char* tv = (char*)kv->tail_v + (size_t)l * R * tail_row * es;
        {
            PROF(COGS_PROF_OTHER);
            COGS_TRY(cogs_k_kv_append(st, dt, (const char*)b.qkv + (size_t)qd_q * es, (const char*)b.qkv + (size_t)(qd_q + kvd) * es, qd,
                                      tk + (size_t)tl * kvd * es, tv + (size_t)tl * kvd * es, (long)tail_row, R, kvd));
        }
        CogsAttnRows a;
        a.Q = b.qkv; a.ldq = qd;
        a.K = kv_row(kv->k, l, kv->max_len, 0, kvd * es); a.V = kv_row(kv->v, l, kv->max_len, 0, kvd * es);
        a.ldk = a.ldv = kvd; a.prefix_len = kv->prefix_len;
        a.tail_k = tk; a.tail_v = tv; a.tail_ld = kvd; a.tail_row = (long)tail_row; a.tail_len = tl + 1;
        a.O = b.att; a.rows = R; a.hq = w.heads; a.hkv = w.kv_heads; a.head_dim = hd;
        a.nsplit = nsplit; a.ws = b.split; a.ws_bytes = b.split_bytes;
        a.tail_slot = tail_slot; a.tail_slot_ld = kv->tail_max;
        PROF(COGS_PROF_ATTN);
        return cogs_k_attention_rows(st, a);
    };
    for (int l = 0; l < w.layers; ++l) {
        const LayerArgs a{R, b.x, false, true, nullptr, nullptr, fp8 ? h->fp8_layers[l] : cogs_llm_fp8_layer{}};
        COGS_TRY(llm_layer(h, st, l, b, a, linear, attend));
    }
    { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_rmsnorm(st, dt, b.x, b.ln, w.final_norm, R, H, w.rms_eps)); }
    CogsGemm g = lm_head_gemm(w, b.ln, R, logits, w.vocab, 0, w.vocab);
    { PROF(COGS_PROF_GEMM); COGS_TRY(linear(g, h->fp8.lm_head_q, h->fp8.lm_head_s)); }
    kv->tail_len = tl + 1;
    return COGS_OK;
}

}  // extern "C"
