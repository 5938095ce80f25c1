// C-ABI layer, vision side: the ViT encoder's launch sequence (one or several frame ranges on their own streams), the
// projector and the RCCL token all-gather. Handle, carver and profiling bracket: capi_internal.h.
#include "capi_internal.h"
#include <stdlib.h>
#include <dlfcn.h>
#include <atomic>

extern "C" {

// ---------------------------------------------------------------- vision encoder

cogs_status cogs_vit_load(cogs_handle h, const cogs_vit_weights* w) {
    if (!h || !w || !w->layer || w->layers <= 0 || w->heads <= 0) return COGS_E_INVALID;
    if (w->hidden % w->heads || (w->hidden / w->heads) % 4) return COGS_E_INVALID;
    const int slab = w->dtype == COGS_DT_BF16 ? 64 : 32;
    if (w->hidden % slab || w->inter_pad % slab || w->patch_pad % slab || w->inter_pad % 4) return COGS_E_INVALID;
    h->vit = *w;
    h->vit_layers.assign(w->layer, w->layer + w->layers);
    h->vit.layer = h->vit_layers.data();
    // VisionRotaryEmbedding(head_dim // 2): inv_freq = 1 / theta^(arange(0, dim, 2)/dim), dim = head_dim/2
    const int hd = w->hidden / w->heads;
    const int dim = hd / 2;
    const int nf = dim / 2;
    std::vector<float> inv(nf);
    for (int i = 0; i < nf; ++i) inv[i] = 1.0f / powf(10000.0f, (float)(2 * i) / (float)dim);
    if (h->vit_inv_freq) (void)hipFree(h->vit_inv_freq);
    if (hipMalloc(&h->vit_inv_freq, nf * sizeof(float)) != hipSuccess) return COGS_E_HIP;
    if (hipMemcpy(h->vit_inv_freq, inv.data(), nf * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return COGS_E_HIP;
    h->vit_nfreq = nf;
    h->vit_ok = true;
    return COGS_OK;
}

// workspace of one frame range of N patches in `nframes` frames (base == nullptr: only `bytes` is meaningful)
struct VitScratch {
    void *xpad, *x, *ln, *big;
    float *rc, *lut;
    int32_t *cu, *lo, *hi;
    size_t bytes;
};
static VitScratch vit_scratch(const cogs_vit_weights& w, int64_t N, int nframes, void* base) {
    const size_t es = esize(w.dtype);
    const int hd = w.hidden / w.heads;
    Carver c(base);
    VitScratch s;
    s.xpad = c.take((size_t)N * w.patch_pad * es);
    s.x = c.take((size_t)N * w.hidden * es);
    s.ln = c.take((size_t)N * w.hidden * es);
    const size_t bigcols = (size_t)(4 * w.hidden > w.inter_pad ? 4 * w.hidden : w.inter_pad);
    s.big = c.take((size_t)N * bigcols * es);  // [qkv | attn_out] then reused as the MLP hidden
    s.rc = (float*)c.take((size_t)N * (hd / 2) * 2 * sizeof(float));   // interleaved (cos, sin) table
    s.cu = (int32_t*)c.take((size_t)(nframes + 1) * sizeof(int32_t));
    s.lo = (int32_t*)c.take((size_t)N * sizeof(int32_t));
    s.hi = (int32_t*)c.take((size_t)N * sizeof(int32_t));
    s.lut = (float*)c.take(28 * 1024);   // rotary position LUT
    s.bytes = c.off;
    return s;
}

cogs_status cogs_vit_set_streams(cogs_handle h, int streams) {
    if (!h || streams < 1 || streams > 4) return COGS_E_INVALID;
    h->vit_streams = streams;
    return COGS_OK;
}

cogs_status cogs_vit_workspace_bytes(cogs_handle h, int64_t n_patches, size_t* bytes) {
    if (!h || !h->vit_ok || !bytes || n_patches <= 0) return COGS_E_INVALID;
    // frames <= patches; size the cu_seqlens array for the worst case
    // + room for the further sets of fixed-size tables when a clip is encoded as up to four frame ranges (cogs_vit_encode)
    *bytes = vit_scratch(h->vit, n_patches, (int)n_patches, nullptr).bytes + 256 * 1024;
    return COGS_OK;
}

// One contiguous run of frames of a clip on one stream. The encoder is queued in three kinds of step -- begin (tables,
// patch embedding), layer(l), finish (post-LayerNorm + merge) -- so that cogs_vit_encode can ALTERNATE the steps of several
// ranges between their streams: queued one whole range after the other (rounds 3-4), the second stream's first kernel
// reached the GPU ~250 launches = 0.9 ms after the first stream's, and ran that much alone at the end -- a tenth of a
// frame-sharded rank's 8.5 ms step.
struct VitRange {
    cogs_handle h; hipStream_t st;
    const void* pixel_values; int pix_dtype;
    std::vector<int64_t> grid, merge;     // [V][3], [V]
    int attn_mode; void* out_tokens; void* ws; size_t ws_bytes;
    // derived by begin()
    int64_t N = 0; int nframes = 0, V = 0;
    VitScratch b{};                       // the range's buffers, carved from ws
    float *stat_part = nullptr, *ln_ab = nullptr;
    bool fold = false, use_lut = false, prescale_q = false, head_major = false;
    int maxpos = 0, max_seq = 0, uniform_seq = 0;
    float scale = 1.f;
    int co_streams = 1;                   // ranges encoded side by side on their own streams (CogsGemm::co_streams)

    cogs_status begin();
    cogs_status layer(int l);
    cogs_status finish();
};

// the projector's two GEMMs on M rows (arguments checked by the callers; ws holds M x out_dim elements); co_streams: streams
// that run a projector of this size side by side
static cogs_status cogs_project_rows(cogs_handle h, hipStream_t st, const void* tokens, int M, void* out, void* ws, int co_streams) {
    if (M <= 0) return COGS_OK;
    const cogs_proj_weights& w = h->proj;
    CogsGemm g; g.dtype = w.dtype; g.co_streams = co_streams;
    g.A = tokens; g.lda = w.in_dim; g.W = w.w1; g.ldw = w.in_dim; g.C = ws; g.ldc = w.out_dim;
    g.bias = w.b1; g.M = M; g.N = w.out_dim; g.K = w.in_dim; g.act = COGS_ACT_GELU_ERF;
    { PROF(COGS_PROF_GEMM); COGS_TRY(cogs_k_gemm(st, g)); }
    CogsGemm g2; g2.dtype = w.dtype; g2.co_streams = co_streams;
    g2.A = ws; g2.lda = w.out_dim; g2.W = w.w2; g2.ldw = w.out_dim; g2.C = out; g2.ldc = w.out_dim;
    g2.bias = w.b2; g2.M = M; g2.N = w.out_dim; g2.K = w.out_dim;
    { PROF(COGS_PROF_GEMM); COGS_TRY(cogs_k_gemm(st, g2)); }
    return COGS_OK;
}

// Frames are independent under block-diagonal attention (per-frame attention, RoPE and 2x2 merge:
// modeling_videollama3_encoder.py:309-312,427,487-501), so a clip is encoded as two halves on two streams: the second
// half's kernels take the CUs the first half's ragged last rounds leave idle (every persistent GEMM launch ends in a
// partly filled round of tiles). Same arithmetic per row, bit-identical tokens (tests/test_gpu_models.py). One rank's
// share of a frame-sharded clip (8 frames of 22 x 42 patches: 145 tiles for the N = 1152 shapes) gains 10 %, the whole
// 64-frame clip 2.7 % (round 4, same box, interleaved: 60.8 -> 59.2 ms; 256 frames at 140 x 280: 47.3 -> 46.5 ms).
// Not while the per-kernel profiler is on: overlapping launches stretch every bracket, so bench.py's `roofline` and
// `breakdown_ms` describe the kernels one at a time. cogs_vit_set_streams(h, 1) or the debug switch vit_split_max switch it off.

// proj_out != NULL: every frame range also runs the projector on its own tokens, on its own stream (cogs_vit_encode_project)
static cogs_status vit_encode_impl(cogs_handle h, cogs_stream stream, const void* pixel_values, int pix_dtype,
                                   const int64_t* grid_sizes, const int64_t* merge_sizes, int V, int attn_mode,
                                   void* out_tokens, void* ws, size_t ws_bytes, void* proj_out, void* proj_ws) {
    if (!h || !h->vit_ok || !pixel_values || !grid_sizes || !merge_sizes || V <= 0 || !out_tokens) return COGS_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    int64_t N = 0, nframes = 0;
    for (int v = 0; v < V; ++v) {
        const int64_t t = grid_sizes[3 * v], gh = grid_sizes[3 * v + 1], gw = grid_sizes[3 * v + 2], ms = merge_sizes[v];
        if (t <= 0 || gh <= 0 || gw <= 0 || ms <= 0 || gh % ms || gw % ms) return COGS_E_INVALID;
        N += t * gh * gw;
        nframes += t;
    }
    const cogs_vit_weights& w = h->vit;
    auto whole = [&]() {
        VitRange r{h, st, pixel_values, pix_dtype, std::vector<int64_t>(grid_sizes, grid_sizes + 3 * V),
                   std::vector<int64_t>(merge_sizes, merge_sizes + V), attn_mode, out_tokens, ws, ws_bytes};
        COGS_TRY(r.begin());
        for (int l = 0; l < w.layers; ++l) COGS_TRY(r.layer(l));
        COGS_TRY(r.finish());
        if (proj_out) {
            int64_t toks = 0;
            for (int v = 0; v < V; ++v) toks += grid_sizes[3 * v] * grid_sizes[3 * v + 1] * grid_sizes[3 * v + 2] / (merge_sizes[v] * merge_sizes[v]);
            COGS_TRY(cogs_project_rows(h, st, out_tokens, (int)toks, proj_out, proj_ws, 1));
        }
        return COGS_OK;
    };
    const int64_t split_max = g_cogs_debug.vit_split_max;
    int S = h->vit_streams;
    if (S > nframes) S = (int)nframes;
    if (S < 2 || h->prof_on || attn_mode != COGS_ATTN_BLOCK_DIAG || N > split_max) return whole();

    // cut the frames into S contiguous runs at the frame boundaries nearest to r / S of the patches
    std::vector<VitRange> R;
    std::vector<int64_t> tok_begin;                       // first token row of every range, then the total
    {
        std::vector<int64_t> frame_rows, frame_v;       // per frame: patches, video
        for (int v = 0; v < V; ++v)
            for (int64_t f = 0; f < grid_sizes[3 * v]; ++f) { frame_rows.push_back(grid_sizes[3 * v + 1] * grid_sizes[3 * v + 2]); frame_v.push_back(v); }
        std::vector<int64_t> cum(nframes + 1, 0);
        for (int64_t f = 0; f < nframes; ++f) cum[f + 1] = cum[f] + frame_rows[f];
        std::vector<int64_t> cuts(1, 0);
        for (int r = 1; r < S; ++r) {
            int64_t best = cuts.back() + 1;
            for (int64_t f = cuts.back() + 1; f <= nframes - (S - r); ++f)
                if (llabs(cum[f] * S - N * r) < llabs(cum[best] * S - N * r)) best = f;
            cuts.push_back(best);
        }
        cuts.push_back(nframes);
        size_t ws_off = 0;
        int64_t tok_off = 0;
        tok_begin.clear();
        const size_t pes = pix_dtype == COGS_DT_BF16 ? 2 : 4;
        bool ok = ws != nullptr;
        for (int r = 0; r < S && ok; ++r) {
            VitRange q{h, nullptr, (const char*)pixel_values + (size_t)cum[cuts[r]] * w.patch_dim * pes, pix_dtype, {}, {}, attn_mode,
                       (char*)out_tokens + (size_t)tok_off * w.hidden * esize(w.dtype), (char*)ws + ws_off, 0};
            int64_t rows = 0, toks = 0;
            for (int64_t f = cuts[r]; f < cuts[r + 1]; ++f) {       // frames -> (t, gh, gw) runs per video
                const int v = (int)frame_v[f];
                if (!q.merge.empty() && q.grid[q.grid.size() - 2] == grid_sizes[3 * v + 1] && q.grid.back() == grid_sizes[3 * v + 2] &&
                    f > cuts[r] && frame_v[f - 1] == v) ++q.grid[q.grid.size() - 3];
                else { q.grid.insert(q.grid.end(), {1, grid_sizes[3 * v + 1], grid_sizes[3 * v + 2]}); q.merge.push_back(merge_sizes[v]); }
                rows += frame_rows[f];
                toks += frame_rows[f] / (merge_sizes[v] * merge_sizes[v]);
            }
            q.ws_bytes = vit_scratch(w, rows, (int)(cuts[r + 1] - cuts[r]), nullptr).bytes;
            ws_off += q.ws_bytes;
            tok_begin.push_back(tok_off);
            tok_off += toks;
            ok = ws_off <= ws_bytes && rows > 0;
            R.push_back(std::move(q));
        }
        tok_begin.push_back(tok_off);
        if (!ok) return whole();
    }
    while ((int)h->aux_streams.size() < S - 1) {          // streams and events of the handle, created once
        hipStream_t s2 = nullptr;
        hipEvent_t e2 = nullptr;
        if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&e2, hipEventDisableTiming) != hipSuccess) {
            if (s2) (void)hipStreamDestroy(s2);       // whatever was created goes back; the clip is encoded on the caller's stream alone
            return whole();
        }
        h->aux_streams.push_back(s2);
        h->ev_joins.push_back(e2);
    }
    if (!h->ev_fork && hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) return whole();
    if (hipEventRecord(h->ev_fork, st) != hipSuccess) return COGS_E_HIP;
    R[0].st = st;
    for (int r = 1; r < S; ++r) {
        R[r].st = h->aux_streams[r - 1];
        if (hipStreamWaitEvent(R[r].st, h->ev_fork, 0) != hipSuccess) return COGS_E_HIP;
    }
    for (int r = 0; r < S; ++r) R[r].co_streams = S;
    cogs_status rc = COGS_OK;
    for (int r = 0; r < S && rc == COGS_OK; ++r) rc = R[r].begin();
    for (int l = 0; l < w.layers && rc == COGS_OK; ++l)
        for (int r = 0; r < S && rc == COGS_OK; ++r) rc = R[r].layer(l);
    for (int r = 0; r < S && rc == COGS_OK; ++r) rc = R[r].finish();
    if (proj_out) {
        // the projector's two GEMMs of a range run behind that range's encoder, on its stream: rows are independent, so the
        // projected tokens are the bits cogs_project gives on the whole clip, and no range waits for the join to be projected
        const size_t tes = (size_t)w.hidden * esize(w.dtype), pes2 = (size_t)h->proj.out_dim * esize(h->proj.dtype);
        for (int r = 0; r < S && rc == COGS_OK; ++r)
            rc = cogs_project_rows(h, R[r].st, (const char*)out_tokens + (size_t)tok_begin[r] * tes, (int)(tok_begin[r + 1] - tok_begin[r]),
                                   (char*)proj_out + (size_t)tok_begin[r] * pes2, (char*)proj_ws + (size_t)tok_begin[r] * pes2, S);
    }
    // join unconditionally: the caller's stream must not run ahead of anything queued on the other ones
    for (int r = 1; r < S; ++r)
        if (hipEventRecord(h->ev_joins[r - 1], R[r].st) != hipSuccess || hipStreamWaitEvent(st, h->ev_joins[r - 1], 0) != hipSuccess) return COGS_E_HIP;
    return rc;
}

cogs_status cogs_vit_encode(cogs_handle h, cogs_stream stream, const void* pixel_values, int pix_dtype,
                            const int64_t* grid_sizes, const int64_t* merge_sizes, int V, int attn_mode,
                            void* out_tokens, void* ws, size_t ws_bytes) {
    return vit_encode_impl(h, stream, pixel_values, pix_dtype, grid_sizes, merge_sizes, V, attn_mode, out_tokens, ws, ws_bytes,
                           nullptr, nullptr);
}

cogs_status cogs_vit_encode_project(cogs_handle h, cogs_stream stream, const void* pixel_values, int pix_dtype,
                                    const int64_t* grid_sizes, const int64_t* merge_sizes, int V, int attn_mode,
                                    void* out_tokens, void* ws, size_t ws_bytes, void* proj_out, void* proj_ws,
                                    size_t proj_ws_bytes) {
    if (!h || !h->proj_ok || !h->vit_ok || !proj_out || !grid_sizes || !merge_sizes || V <= 0) return COGS_E_INVALID;
    if (h->proj.in_dim != h->vit.hidden || h->proj.dtype != h->vit.dtype) return COGS_E_INVALID;
    int64_t toks = 0;
    for (int v = 0; v < V; ++v) {
        const int64_t ms = merge_sizes[v];
        if (ms <= 0) return COGS_E_INVALID;
        toks += grid_sizes[3 * v] * grid_sizes[3 * v + 1] * grid_sizes[3 * v + 2] / (ms * ms);
    }
    if (!proj_ws || proj_ws_bytes < (size_t)toks * h->proj.out_dim * esize(h->proj.dtype)) return COGS_E_WORKSPACE;
    return vit_encode_impl(h, stream, pixel_values, pix_dtype, grid_sizes, merge_sizes, V, attn_mode, out_tokens, ws, ws_bytes,
                           proj_out, proj_ws);
}

cogs_status VitRange::begin() {
    const cogs_vit_weights& w = h->vit;
    const int dt = w.dtype;
    const int H = w.hidden, hd = H / w.heads;
    V = (int)merge.size();
    const int64_t* grid_sizes = grid.data();
    const int64_t* merge_sizes = merge.data();
    N = 0; nframes = 0;
    for (int v = 0; v < V; ++v) {
        const int64_t t = grid_sizes[3 * v], gh = grid_sizes[3 * v + 1], gw = grid_sizes[3 * v + 2], ms = merge_sizes[v];
        if (t <= 0 || gh <= 0 || gw <= 0 || ms <= 0 || gh % ms || gw % ms) return COGS_E_INVALID;
        N += t * gh * gw;
        nframes += (int)t;
    }
    if (N > 0x7fffffff) return COGS_E_INVALID;
    b = vit_scratch(w, N, nframes, ws);
    if (!ws || ws_bytes < b.bytes) return COGS_E_WORKSPACE;
    // LayerNorm folded into the GEMMs (bf16 production path, cogs_vit_layer.qkv_c ...): the buffer that would hold LN(x)
    // carries the per-row partial statistics [N][H/64][2] and the per-row (rstd, -rstd*mean) [N][2] instead
    fold = dt == COGS_DT_BF16 && H % 64 == 0;
    for (int l = 0; l < w.layers && fold; ++l) {
        const cogs_vit_layer& L = h->vit_layers[l];
        fold = L.qkv_c && L.fc1_c;
    }
    stat_part = (float*)b.ln;
    ln_ab = stat_part + (size_t)N * (H / 64) * 2;

    // rotary position LUT for the ping-pong QKV GEMM (bf16, block-diagonal): (cos, sin)[pos][freq], kept in LDS there
    maxpos = 0;
    for (int v = 0; v < V; ++v) {
        const int gh = (int)grid_sizes[3 * v + 1], gw = (int)grid_sizes[3 * v + 2];
        maxpos = gh > maxpos ? gh : maxpos;
        maxpos = gw > maxpos ? gw : maxpos;
    }
    use_lut = dt == COGS_DT_BF16 && attn_mode == COGS_ATTN_BLOCK_DIAG && hd % 4 == 0 && maxpos * (hd / 4) * 8 <= 27 * 1024;

    // cu_seqlens (:439-440), same-frame ranges for the eager-global mode, rotary tables (:405-434): all written by
    // kernels on `st` from the grid -- no host staging, so back-to-back encodes with different grids cannot race
    max_seq = 0; uniform_seq = 0;
    {
        bool alike = true;
        for (int v = 1; v < V; ++v)
            alike = alike && grid_sizes[3 * v + 1] * grid_sizes[3 * v + 2] == grid_sizes[1] * grid_sizes[2];
        if (alike) uniform_seq = (int)(grid_sizes[1] * grid_sizes[2]);
    }
    {
        int64_t row = 0;
        int frame0 = 0;
        const bool need_rows = attn_mode == COGS_ATTN_REF_EAGER_GLOBAL;
        for (int v = 0; v < V; ++v) {
            const int t = (int)grid_sizes[3 * v], gh = (int)grid_sizes[3 * v + 1], gw = (int)grid_sizes[3 * v + 2];
            const int per = gh * gw;
            if (per > max_seq) max_seq = per;
            { PROF(COGS_PROF_OTHER); COGS_TRY(cogs_k_vit_rope_table(st, b.rc, nullptr, (int)row, t, gh, gw, (int)merge_sizes[v], h->vit_inv_freq, h->vit_nfreq)); }
            if (use_lut) {   // `lo` is free in block-diagonal mode: per-row positions; the LUT itself once (first video)
                PROF(COGS_PROF_OTHER);
                COGS_TRY(cogs_k_vit_rope_lut(st, b.lo, (int)row, t, gh, gw, (int)merge_sizes[v], v == 0 ? b.lut : nullptr, maxpos,
                                             h->vit_inv_freq, h->vit_nfreq));
            }
            { PROF(COGS_PROF_OTHER); COGS_TRY(cogs_k_vit_segments(st, b.cu, need_rows ? b.lo : nullptr, need_rows ? b.hi : nullptr, (int)row, frame0, t, per)); }
            row += (int64_t)t * per;
            frame0 += t;
        }
    }

    // patch embed: conv2d k=s=14 == GEMM over the 588-element rows (:202-210)
    { PROF(COGS_PROF_OTHER); COGS_TRY(cogs_k_pack_rows(st, pix_dtype, dt, pixel_values, w.patch_dim, b.xpad, w.patch_pad, (int)N, w.patch_dim, w.patch_pad)); }
    {
        CogsGemm g; g.dtype = dt; g.co_streams = co_streams;
        g.A = b.xpad; g.lda = w.patch_pad; g.W = w.patch_w; g.ldw = w.patch_pad; g.C = b.x; g.ldc = H;
        g.bias = w.patch_b; g.M = (int)N; g.N = H; g.K = w.patch_pad;
        if (fold) g.row_stats = stat_part;
        { PROF(COGS_PROF_GEMM); COGS_TRY(cogs_k_gemm(st, g)); }
    }
    scale = 1.0f / sqrtf((float)hd);
    // bf16 MFMA attention kernels take Q pre-multiplied by scale*log2(e): the QKV GEMM epilogue folds the factor in
    // before its single rounding (same relative rounding error as rounding q itself) and the softmax needs no
    // per-score multiply. Not in the parity modes (fp32, or the eager-global bias mode).
    prescale_q = dt == COGS_DT_BF16 && attn_mode == COGS_ATTN_BLOCK_DIAG && (hd == 72 || hd == 128);
    // Round 5: the production path keeps q, k, v HEAD-major between the QKV GEMM and the attention kernel --
    // [q | k | v][head][row][hd] in the same N x 3H elements -- so that a (frame, head) block of K / V is one contiguous
    // run and the attention kernel's LDS-DMA pieces are whole 128-byte lines (csrc/gemm_epilogue.h EPI_HM, csrc/attn_vit.hip).
    // Only that kernel reads the layout; the parity modes (fp32, eager-global) stay token-major.
    head_major = prescale_q && hd == 72 && g_cogs_debug.gemm_headmajor != 0 && g_cogs_debug.attn_vit != 0 &&
                 (double)N * H * 2.0 < 4294967296.0;
    return COGS_OK;
}

cogs_status VitRange::layer(int l) {
    const cogs_vit_weights& w = h->vit;
    const int dt = w.dtype;
    const size_t es = esize(dt);
    const int H = w.hidden, hd = H / w.heads;
    char* qkv = (char*)b.big;
    char* att = qkv + (size_t)N * 3 * H * es;
    const cogs_vit_layer& L = h->vit_layers[l];
    if (fold) { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_ln_finalize(st, stat_part, (int)N, H / 64, H, w.ln_eps, ln_ab)); }
    else { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_layernorm(st, dt, b.x, b.ln, L.ln1_g, L.ln1_b, (int)N, H, w.ln_eps)); }
    {
        CogsGemm g; g.dtype = dt; g.co_streams = co_streams;
        g.A = fold ? b.x : b.ln; g.lda = H; g.W = L.qkv_w; g.ldw = H; g.C = qkv; g.ldc = 3 * H;
        g.M = (int)N; g.N = 3 * H; g.K = H;
        if (fold) { g.ln_ab = ln_ab; g.col_c = L.qkv_c; }
        else g.bias = L.qkv_b;
        g.rope_cos = b.rc; g.rope_sin = nullptr; g.rope_cols = 2 * H; g.head_dim = hd;
        if (prescale_q) { g.q_scale = scale * 1.4426950408889634f; g.q_cols = H; }
        if (use_lut) { g.rope_lut = b.lut; g.rope_rowpos = b.lo; g.rope_maxpos = maxpos; }
        if (head_major) { g.hm_rows = N; g.hm_cols = H; }
        { PROF(COGS_PROF_GEMM); COGS_TRY(cogs_k_gemm(st, g)); }
    }
    {
        CogsAttn a; a.dtype = dt;
        a.Q = qkv; a.K = qkv + (size_t)H * es; a.V = qkv + (size_t)2 * H * es; a.O = att;
        a.ldq = a.ldk = a.ldv = 3 * H; a.ldo = H;
        if (head_major) {
            a.K = qkv + (size_t)N * H * es; a.V = qkv + (size_t)2 * N * H * es;
            a.ldq = a.ldk = a.ldv = hd; a.head_stride = (long)N * hd;
        }
        a.q_len = (int)N; a.kv_len = (int)N; a.hq = a.hkv = w.heads; a.head_dim = hd; a.scale = scale;
        a.q_prescaled = prescale_q;
        if (attn_mode == COGS_ATTN_REF_EAGER_GLOBAL) { a.row_lo = b.lo; a.row_hi = b.hi; a.bias = 1.0f; }
        else {
            a.cu_seqlens = b.cu; a.nseg = nframes; a.max_seqlen = max_seq;
            a.uniform_seqlen = uniform_seq;      // all frames alike (one video, or videos of one grid): see attn_vit.hip
        }
        { PROF(COGS_PROF_ATTN); COGS_TRY(cogs_k_attention(st, a)); }
    }
    {
        CogsGemm g; g.dtype = dt; g.co_streams = co_streams;
        g.A = att; g.lda = H; g.W = L.o_w; g.ldw = H; g.C = b.x; g.ldc = H;
        g.bias = L.o_b; g.residual = b.x; g.ldr = H; g.M = (int)N; g.N = H; g.K = H;
        if (fold) g.row_stats = stat_part;
        { PROF(COGS_PROF_GEMM); COGS_TRY(cogs_k_gemm(st, g)); }
    }
    if (fold) { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_ln_finalize(st, stat_part, (int)N, H / 64, H, w.ln_eps, ln_ab)); }
    else { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_layernorm(st, dt, b.x, b.ln, L.ln2_g, L.ln2_b, (int)N, H, w.ln_eps)); }
    {
        CogsGemm g; g.dtype = dt; g.co_streams = co_streams;
        g.A = fold ? b.x : b.ln; g.lda = H; g.W = L.fc1_w; g.ldw = H; g.C = b.big; g.ldc = w.inter_pad;
        g.M = (int)N; g.N = w.inter_pad; g.K = H; g.act = COGS_ACT_GELU_TANH;
        if (fold) { g.ln_ab = ln_ab; g.col_c = L.fc1_c; }
        else g.bias = L.fc1_b;
        { PROF(COGS_PROF_GEMM); COGS_TRY(cogs_k_gemm(st, g)); }
    }
    {
        CogsGemm g; g.dtype = dt; g.co_streams = co_streams;
        g.A = b.big; g.lda = w.inter_pad; g.W = L.fc2_w; g.ldw = w.inter_pad; g.C = b.x; g.ldc = H;
        g.bias = L.fc2_b; g.residual = b.x; g.ldr = H; g.M = (int)N; g.N = H; g.K = w.inter_pad;
        if (fold && l + 1 < w.layers) g.row_stats = stat_part;     // the last layer feeds post_layernorm (own kernel)
        { PROF(COGS_PROF_GEMM); COGS_TRY(cogs_k_gemm(st, g)); }
    }
    return COGS_OK;
}

// post_layernorm + per-video 2x2 merge (:482-510)
cogs_status VitRange::finish() {
    const cogs_vit_weights& w = h->vit;
    const int dt = w.dtype;
    const size_t es = esize(dt);
    const int H = w.hidden;
    int64_t row = 0, orow = 0;
    for (int v = 0; v < V; ++v) {
        const int64_t n = grid[3 * v] * grid[3 * v + 1] * grid[3 * v + 2];
        const int grp = (int)(merge[v] * merge[v]);
        { PROF(COGS_PROF_NORM); COGS_TRY(cogs_k_ln_merge(st, dt, (char*)b.x + (size_t)row * H * es, (char*)out_tokens + (size_t)orow * H * es,
                                 w.post_ln_g, w.post_ln_b, (int)(n / grp), grp, H, w.ln_eps)); }
        row += n;
        orow += n / grp;
    }
    return COGS_OK;
}

// ---------------------------------------------------------------- multi-GPU
// RCCL is bound at first use: libcogs_hip.so itself does not link against it (a single-GPU user never loads it)
typedef int (*cogs_nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
static cogs_nccl_allgather_fn cogs_bind_allgather() {
    static std::atomic<int> state{0};      // 0 = not tried, 1 = bound, -1 = unavailable
    static cogs_nccl_allgather_fn fn = nullptr;
    const int s = state.load(std::memory_order_acquire);
    if (s != 0) return s > 0 ? fn : nullptr;
    void* lib = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (lib) break;
    }
    cogs_nccl_allgather_fn f = lib ? (cogs_nccl_allgather_fn)dlsym(lib, "ncclAllGather") : nullptr;
    fn = f;
    state.store(f ? 1 : -1, std::memory_order_release);
    return f;
}
cogs_status cogs_allgather_tokens(cogs_stream stream, void* nccl_comm, const void* local, size_t local_rows,
                                  size_t row_bytes, void* global) {
    if (!nccl_comm || !local || !global || local_rows == 0 || row_bytes == 0) return COGS_E_INVALID;
    cogs_nccl_allgather_fn f = cogs_bind_allgather();
    if (!f) return COGS_E_UNSUPPORTED;
    const int nccl_uint8 = 1;              // ncclUint8 (rccl.h): the payload is moved as bytes, whatever its dtype
    return f(local, global, local_rows * row_bytes, nccl_uint8, nccl_comm, (hipStream_t)stream) == 0 ? COGS_OK : COGS_E_HIP;
}

cogs_status cogs_proj_load(cogs_handle h, const cogs_proj_weights* w) {
    if (!h || !w || !w->w1 || !w->w2) return COGS_E_INVALID;
    const int slab = w->dtype == COGS_DT_BF16 ? 64 : 32;
    if (w->in_dim % slab || w->out_dim % slab) return COGS_E_INVALID;
    h->proj = *w;
    h->proj_ok = true;
    return COGS_OK;
}

cogs_status cogs_project(cogs_handle h, cogs_stream stream, const void* tokens, int M, void* out, void* ws,
                         size_t ws_bytes) {
    if (!h || !h->proj_ok || !tokens || !out || M <= 0) return COGS_E_INVALID;
    const cogs_proj_weights& w = h->proj;
    if (!ws || ws_bytes < (size_t)M * w.out_dim * esize(w.dtype)) return COGS_E_WORKSPACE;
    return cogs_project_rows(h, (hipStream_t)stream, tokens, M, out, ws, 1);
}

}  // extern "C"
