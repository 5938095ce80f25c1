// Launch plan of cogs_k_attention and cogs_k_attention_rows: which kernel a descriptor gets, in which instantiation, on which
// grid, with which derived kernel arguments, which combine step follows and how large the partial buffer must be -- or the
// status the call is rejected with. Host integer arithmetic only: no HIP, compiles with the host C++ compiler
// (tests/test_attn_plan.py pins it on the CPU against tests/golden/attn_plan.json).
#pragma once
#include <stddef.h>
#include "status.h"

// the attn_* / llm_* switches of debug.h that the plan reads, at their shipped defaults (attn_uniform_hint is not one of
// them: capi.hip turns it into the descriptor's uniform_seqlen)
struct AttnTuning {
    long long attn_vit = 2, attn_vit_early = 0, attn_vit_len = 1, attn_decode = 1, attn_combine32 = 1, attn_prefill_dma = 1,
              attn_light_first = 0, attn_nq = 0, llm_split_keys = 0;
};

// what the decision depends on of a CogsAttn (kernels.h): no pointers, only whether they are there
struct AttnQuery {
    bool bf16 = true;            // dtype: COGS_DT_BF16 (else fp32)
    int head_dim = 0, q_len = 0, kv_len = 0, hq = 1, hkv = 1;
    long ldq = 0, ldk = 0, ldv = 0, ldo = 0, head_stride = 0;
    bool has_cu = false, has_row_lo = false, has_ws = false;
    int nseg = 1, max_seqlen = 0, uniform_seqlen = 0;
    int causal = 0, q_pos0 = 0;  // (q_pos0: the decode kernel's key count is min(q_pos0 + 1, kv_len), and none is an error)
    int q_prescaled = 0, force_rowwise = 0, nsplit = 1;
    size_t ws_bytes = 0;
};

// ... and of a CogsAttnRows
struct AttnRowsQuery {
    int rows = 0, hq = 1, hkv = 1, head_dim = 0, prefix_len = 0, tail_len = 0;
    long ldq = 0, ldk = 0, ldv = 0, tail_ld = 0, tail_row = 0, tail_slot_ld = 0;
    bool has_slot = false, has_ws = false;
    int nsplit = 1;
    size_t ws_bytes = 0;
};

enum { ATTN_COMBINE_NONE = 0, ATTN_COMBINE_HEAD = 1, ATTN_COMBINE_SLICE32 = 2 };

struct AttnPlan {
    int status = COGS_OK;        // != COGS_OK: nothing is launched and no other field is meaningful
    // the attn_last_kernel numbering: 1 general MFMA kernel, 2 ViT unpipelined, 3 ViT pipelined (token-major K / V), 4 single-token
    // decode (+ combine), 5 prompt LDS-DMA kernel, 7 row-wise kernel, 8 ViT pipelined, head-major. 0: the multi-row decode step
    // (cogs_attention_rows reports none)
    int kernel = 0;
    // the instantiation
    int hd = 0, nq = 0, pre = 0;         // kernel 1: attn_fwd_bf16_kernel<hd, nq, pre> (threads = block_x)
    int vit_pipe = 0, vit_r = 0, vit_nlb = 0;   // kernels 3 / 8: attn_vit_pipe_kernel<72, vit_r, vit_nlb> ...
    int vit_end = 0;                     //   ... and what attn_vit_last_end reports: 10 vit_r + vit_nlb (0: the run-time form)
    int rows_slot = 0;                   // multi-row step: attn_decode_kernel<true, rows_slot>
    int grid_x = 0, grid_y = 1, grid_z = 1, block_x = 0;
    // kernel arguments the launcher derives (AttnArgs / VitAttnArgs / DecodeAttnArgs)
    int nsplit = 1, gqa_pack = 0, heavy_first = 0, q_prescaled = 0;
    int nqb = 0, uniform_len = 0, xcd_order = 0, early_prefetch = 0;
    long head_stride = 0;
    int kend = 0, gsz = 0, ntile = 1;    // decode kernels: visible (shared) keys, query heads per kv head, column tiles per kv head
    // the combine step behind a key-split launch: `parts` partials of q_len x heads slots
    int combine = ATTN_COMBINE_NONE, combine_x = 0, combine_y = 1, combine_z = 1, parts = 0;
    size_t ws_need = 0;          // bytes of the partial buffer (0: none): [parts][slots][head_dim] unnormalised outputs, then ...
    size_t part_ml_off = 0;      //   ... from this float on [parts][slots][2] (running maximum, sum)
    int nseg = 1;                // segments the general and row-wise kernels walk (1 without cu_seqlens)
};

// Bytes of the key-split partial buffer: per partial and (row, head) slot head_dim unnormalised fp32 outputs + (running maximum,
// sum). cogs_attention: parts = nsplit, rows = q_len; cogs_attention_rows: parts = nsplit + 1 (the rows' tails are one more)
inline size_t cogs_attn_split_ws_bytes(int parts, int rows, int hq, int head_dim) {
    return (size_t)parts * rows * hq * (head_dim + 2) * sizeof(float);
}

// splits of the single-token decode attention at context `ctx`
inline int cogs_attn_nsplit(int ctx, const AttnTuning& t) {
    // decode attention: the keys are split over workgroups (x kv heads) and combined by a second kernel
    // measured (ms/token, 7B, kv heads 4): context 15 360: 256 keys per split 3.62, 128: 3.67, 64: 3.66, 512: 3.72;
    // context 2 048: 256: 3.51, 128: 3.42, 64: 3.39 -- i.e. at least ~32 splits, of 64..256 keys
    // => at least 32 splits while a split keeps 64 keys, 256 keys per split beyond that (monotonic in ctx: the
    // workspace is sized with the largest context)
    const int env_keys = (int)t.llm_split_keys;
    int n;
    if (env_keys > 0) n = (ctx + env_keys - 1) / env_keys;
    else {
        n = (ctx + 255) / 256;
        if (n < 32) n = 32;
        const int cap = (ctx + 63) / 64;
        if (n > cap) n = cap;
    }
    if (n < 1) n = 1;
    if (n > 128) n = 128;
    return n;
}

// the single-row split rule; the rows' tails are one more partial (<= 128 in all)
inline int cogs_attn_rows_nsplit(int prefix_len, const AttnTuning& t) {
    const int n = cogs_attn_nsplit(prefix_len, t);
    return n > 127 ? 127 : n;
}

// the combine step of `parts` partials over q_len x heads slots
inline void cogs_plan_combine(AttnPlan& plan, int parts, int q_len, int heads, int head_dim, const AttnTuning& t) {
    plan.parts = parts;
    plan.combine_x = q_len; plan.combine_y = heads;
    if (head_dim % 32 == 0 && t.attn_combine32 != 0) { plan.combine = ATTN_COMBINE_SLICE32; plan.combine_z = head_dim / 32; }
    else plan.combine = ATTN_COMBINE_HEAD;
}

// the encoder's kernels (attn_vit.hip): block-diagonal bf16 attention with pre-scaled Q, hd 72, hq == hkv
inline AttnPlan cogs_plan_attention_vit(const AttnQuery& q, const AttnTuning& t) {
    AttnPlan plan;
    auto reject = [&](int status) { plan = AttnPlan{}; plan.status = status; return plan; };
    if (q.head_dim != 72 || !q.has_cu || q.nseg <= 0 || q.hq != q.hkv) return reject(COGS_E_UNSUPPORTED);
    if (q.ldq % 8 || q.ldk % 8 || q.ldv % 8 || q.ldo % 8) return reject(COGS_E_INVALID);
    plan.nqb = (q.max_seqlen + 127) / 128;
    plan.head_stride = q.head_stride > 0 ? q.head_stride : 72;
    if (q.head_stride > 0 && (q.ldq != 72 || q.ldk != 72 || q.ldv != 72)) return reject(COGS_E_INVALID);
    plan.uniform_len = (q.uniform_seqlen > 0 && (long)q.uniform_seqlen * q.nseg == q.q_len && q.uniform_seqlen == q.max_seqlen)
                           ? q.uniform_seqlen : 0;
    if (q.nseg > 65535 || q.hq > 65535 || (long)plan.nqb * 8 > 0x7fffffffL) return reject(COGS_E_INVALID);
    plan.xcd_order = q.hq % 8 == 0;
    if (plan.xcd_order) { plan.grid_x = plan.nqb * 8; plan.grid_y = q.hq / 8; }
    else { plan.grid_x = plan.nqb; plan.grid_y = q.hq; }
    plan.grid_z = q.nseg;
    plan.block_x = 256;
    plan.early_prefetch = (int)t.attn_vit_early;
    if (t.attn_vit == 1 || q.ldk != q.ldv) { plan.kernel = 2; return plan; }      // attn_vit = 1: unpipelined (A/B runs)
    plan.kernel = q.head_stride > 0 ? 8 : 3;
    plan.vit_pipe = 1;
    // one video (all segments alike, 4 tiles or more): the instantiation whose ragged end has this length's shape
    const int nt = (plan.uniform_len + 63) >> 6;
    plan.vit_r = (t.attn_vit_len != 0 && plan.uniform_len > 0 && nt >= 4) ? 4 + ((nt - 4) & 3) : 0;
    plan.vit_nlb = plan.vit_r ? (plan.uniform_len - 64 * (nt - 1) > 32 ? 2 : 1) : 0;
    plan.vit_end = plan.vit_r * 10 + plan.vit_nlb;
    return plan;
}

inline AttnPlan cogs_plan_attention(const AttnQuery& q, const AttnTuning& t) {
    AttnPlan plan;
    auto reject = [&](int status) { plan = AttnPlan{}; plan.status = status; return plan; };
    if (q.q_len <= 0 || q.hq <= 0 || q.hkv <= 0 || q.hq % q.hkv != 0) return reject(COGS_E_INVALID);
    if (q.head_dim > 256 || q.head_dim % 8 != 0) return reject(COGS_E_UNSUPPORTED);
    // the encoder's production shape (per-frame segments, hd 72, pre-scaled Q, no masks) has its own kernel
    // (attn_vit = 0: A/B runs only)
    if (q.bf16 && !q.force_rowwise && q.head_dim == 72 && q.q_prescaled && q.has_cu && !q.has_row_lo && !q.causal && q.nsplit <= 1 &&
        q.hq == q.hkv && q.ldo % 8 == 0 && t.attn_vit != 0)
        return cogs_plan_attention_vit(q, t);
    if (q.head_stride > 0) return reject(COGS_E_UNSUPPORTED);      // head-major Q / K / V: the encoder's production kernel only
    plan.nseg = q.has_cu ? q.nseg : 1;
    if (!(q.bf16 && !q.force_rowwise && (q.head_dim == 72 || q.head_dim == 128))) {
        plan.kernel = 7;                                           // one wave per (query row, head)
        plan.grid_x = q.q_len; plan.grid_y = q.hq; plan.block_x = 64;
        return plan;
    }
    if (q.ldq % 8 || q.ldk % 8 || q.ldv % 8 || q.ldo % 4) return reject(COGS_E_INVALID);
    const int max_len = q.has_cu ? q.max_seqlen : q.q_len;
    const int qtiles = (max_len + 127) / 128;
    if (q.nsplit > 1) {
        if (q.has_cu || q.has_row_lo || q.nsplit > 128) return reject(COGS_E_UNSUPPORTED);
        plan.ws_need = cogs_attn_split_ws_bytes(q.nsplit, q.q_len, q.hq, q.head_dim);
        if (!q.has_ws || q.ws_bytes < plan.ws_need) return reject(COGS_E_WORKSPACE);
        plan.nsplit = q.nsplit;
        plan.part_ml_off = (size_t)q.nsplit * q.q_len * q.hq * q.head_dim;
    }
    plan.gqa_pack = q.q_len == 1 && q.hq / q.hkv <= 16 && !q.has_cu;
    plan.grid_x = qtiles * plan.nsplit; plan.grid_y = plan.gqa_pack ? q.hkv : q.hq; plan.grid_z = plan.nseg;
    plan.heavy_first = (q.causal && !q.has_cu && q.q_len > 128 && t.attn_light_first != 1) ? 1 : 0;   // attn_light_first: A/B runs only
    if (q.q_prescaled && q.has_row_lo) return reject(COGS_E_UNSUPPORTED);   // the bias mode is parity-only and unscaled
    const bool pre = q.q_prescaled != 0;
    plan.q_prescaled = pre;
    if (plan.nsplit > 1) cogs_plan_combine(plan, plan.nsplit, q.q_len, q.hq, q.head_dim, t);
    // (every causal pre-scaled hd-128 call, whatever its length: a prompt continued behind a cached prefix with fewer than 128
    // new rows must run the same per-row arithmetic as the full prompt -- PrefixKV's transparency, tests/test_gpu_models.py --
    // and since round 5 this kernel's running maximum is no longer the general kernel's)
    // (attn_prefill_dma = 0: A/B runs only)
    if (q.head_dim == 128 && pre && q.causal && plan.nsplit == 1 && !plan.gqa_pack && !q.has_row_lo && t.attn_prefill_dma != 0 &&
        q.ldo % 8 == 0) {
        // (two more forms were built, tested at full size and measured slower -- a ping-pong form, 1.89 vs 1.81-1.86 ms per layer
        // at 15 395 tokens, and 64 query rows per wave, 2.94 vs 1.97 ms: tools/experiments/attn_prefill_variants.hip)
        plan.kernel = 5;
        plan.block_x = 256;
        return plan;
    }
    // the generated tokens' attention (one query row, key-split) has its own kernel: every wave owns whole tiles
    // (attn_decode = 0: A/B runs only)
    if (q.head_dim == 128 && q.q_len == 1 && plan.nsplit > 1 && plan.gqa_pack && pre && t.attn_decode != 0) {
        plan.kend = q.causal ? (q.q_pos0 + 1 < q.kv_len ? q.q_pos0 + 1 : q.kv_len) : q.kv_len;
        if (plan.kend < 1) return reject(COGS_E_INVALID);
        // (the kernel divides tiles x splits in unsigned 32 bits)
        if ((long)((plan.kend + 63) >> 6) * (plan.nsplit + 1) > 0x7fffffffL) return reject(COGS_E_INVALID);
        plan.kernel = 4;
        plan.gsz = q.hq / q.hkv;
        plan.grid_x = plan.nsplit; plan.grid_y = q.hkv; plan.grid_z = 1; plan.block_x = 256;
        return plan;
    }
    plan.kernel = 1;
    plan.hd = q.head_dim;
    // 8 waves x 16 rows: measured faster for hd 128 (no spills, 4 waves per SIMD: causal prefill 2.58 -> 2.29 ms
    // at 15k tokens), slower for hd 72 (0.49 -> 0.52 ms: its fragment reads make the LDS the busiest unit)
    // (with pre-scaled Q the 4-wave hd 128 kernel needs 243 VGPRs and no longer spills: 2.34 -> 2.26 ms, so the
    // light variant is only the default for the classic softmax)
    const bool light = t.attn_nq ? t.attn_nq == 1 : (q.head_dim == 128 && !q.q_prescaled);
    plan.nq = light && !plan.gqa_pack ? 1 : 2;
    plan.pre = pre;
    plan.block_x = plan.nq == 1 ? 512 : 256;
    return plan;
}

// `rows` query rows in lockstep over one shared prompt (cogs_attention_rows, include/cogs.h): workgroups [0, nsplit * ntile)
// run the key splits of the shared keys per tile of 16 query columns, `rows` more run one row's own tail each, as partial
// nsplit; one combine over the nsplit + 1 partials of rows * hq (row, head) slots
inline AttnPlan cogs_plan_attention_rows(const AttnRowsQuery& q, const AttnTuning& t) {
    AttnPlan plan;
    auto reject = [&](int status) { plan = AttnPlan{}; plan.status = status; return plan; };
    if (q.nsplit < 1 || q.nsplit > 127) return reject(COGS_E_INVALID);
    plan.ws_need = cogs_attn_split_ws_bytes(q.nsplit + 1, q.rows, q.hq, q.head_dim);
    if (!q.has_ws || q.ws_bytes < plan.ws_need) return reject(COGS_E_WORKSPACE);
    if (q.head_dim != 128 || q.hkv < 1 || q.hq % q.hkv || q.hq / q.hkv > 16 || q.rows < 1 || q.rows > 16) return reject(COGS_E_UNSUPPORTED);
    if (q.prefix_len < 1 || q.tail_len < 1) return reject(COGS_E_INVALID);
    if (q.ldk % 8 || q.ldv % 8 || q.ldq % 8 || q.tail_ld % 8 || q.tail_row % 8) return reject(COGS_E_INVALID);
    plan.kend = q.prefix_len;
    if ((long)((plan.kend + 63) >> 6) * (q.nsplit + 1) > 0x7fffffffL) return reject(COGS_E_INVALID);
    if (q.has_slot && q.tail_slot_ld < q.tail_len) return reject(COGS_E_INVALID);
    // (this was cogs_k_attention_combine's own `heads >= 1` check, behind the decode-rows launch: same status, now before any launch)
    if (q.rows * q.hq < 1) return reject(COGS_E_INVALID);
    plan.part_ml_off = (size_t)(q.nsplit + 1) * q.rows * q.hq * q.head_dim;
    plan.rows_slot = q.has_slot;
    plan.nsplit = q.nsplit;
    plan.gsz = q.hq / q.hkv;
    plan.ntile = (q.rows * plan.gsz + 15) / 16;
    plan.grid_x = q.nsplit * plan.ntile + q.rows; plan.grid_y = q.hkv; plan.block_x = 256;
    cogs_plan_combine(plan, q.nsplit + 1, 1, q.rows * q.hq, q.head_dim, t);
    return plan;
}
