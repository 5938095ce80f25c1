// C entry points over csrc/attn_plan.h for tests/test_attn_plan.py (built with the host C++ compiler, loaded with ctypes)
#include "attn_plan.h"

namespace {
constexpr int NT = 9;
long long* fields(AttnTuning& t, int i) {
    long long* f[] = {&t.attn_vit, &t.attn_vit_early, &t.attn_vit_len, &t.attn_decode, &t.attn_combine32, &t.attn_prefill_dma,
                      &t.attn_light_first, &t.attn_nq, &t.llm_split_keys};
    return f[i];
}
AttnTuning tuning(const long long* v) {
    AttnTuning t;
    for (int i = 0; i < NT; ++i) *fields(t, i) = v[i];
    return t;
}
void put(const AttnPlan& p, long long* o) {
    const long long v[] = {p.status, p.kernel, p.hd, p.nq, p.pre, p.vit_pipe, p.vit_r, p.vit_nlb, p.vit_end, p.rows_slot,
                           p.grid_x, p.grid_y, p.grid_z, p.block_x, p.nsplit, p.gqa_pack, p.heavy_first, p.q_prescaled,
                           p.nqb, p.uniform_len, p.xcd_order, p.early_prefetch, p.head_stride, p.kend, p.gsz, p.ntile, p.combine,
                           p.combine_x, p.combine_y, p.combine_z, p.parts, (long long)p.ws_need, (long long)p.part_ml_off, p.nseg};
    for (int i = 0; i < 34; ++i) o[i] = v[i];
}
}  // namespace

extern "C" const char* attn_tuning_names() {
    return "attn_vit attn_vit_early attn_vit_len attn_decode attn_combine32 attn_prefill_dma attn_light_first attn_nq llm_split_keys";
}
extern "C" void attn_tuning_defaults(long long* out) {
    AttnTuning t;
    for (int i = 0; i < NT; ++i) out[i] = *fields(t, i);
}
extern "C" const char* attn_plan_names() {
    return "status kernel hd nq pre vit_pipe vit_r vit_nlb vit_end rows_slot grid_x grid_y grid_z block_x nsplit gqa_pack "
           "heavy_first q_prescaled nqb uniform_len xcd_order early_prefetch head_stride kend gsz ntile combine combine_x "
           "combine_y combine_z parts ws_need part_ml_off nseg";
}
extern "C" const char* attn_query_names() {
    return "bf16 head_dim q_len kv_len hq hkv ldq ldk ldv ldo head_stride has_cu has_row_lo has_ws nseg max_seqlen uniform_seqlen "
           "causal q_pos0 q_prescaled force_rowwise nsplit ws_bytes";
}
extern "C" void plan_attention(const long long* v, const long long* tun, long long* out) {
    AttnQuery q;
    q.bf16 = v[0] != 0; q.head_dim = (int)v[1]; q.q_len = (int)v[2]; q.kv_len = (int)v[3]; q.hq = (int)v[4]; q.hkv = (int)v[5];
    q.ldq = (long)v[6]; q.ldk = (long)v[7]; q.ldv = (long)v[8]; q.ldo = (long)v[9]; q.head_stride = (long)v[10];
    q.has_cu = v[11] != 0; q.has_row_lo = v[12] != 0; q.has_ws = v[13] != 0;
    q.nseg = (int)v[14]; q.max_seqlen = (int)v[15]; q.uniform_seqlen = (int)v[16]; q.causal = (int)v[17]; q.q_pos0 = (int)v[18];
    q.q_prescaled = (int)v[19]; q.force_rowwise = (int)v[20]; q.nsplit = (int)v[21]; q.ws_bytes = (size_t)v[22];
    put(cogs_plan_attention(q, tuning(tun)), out);
}
extern "C" const char* attn_rows_query_names() {
    return "rows hq hkv head_dim prefix_len tail_len ldq ldk ldv tail_ld tail_row tail_slot_ld has_slot has_ws nsplit ws_bytes";
}
extern "C" void plan_attention_rows(const long long* v, const long long* tun, long long* out) {
    AttnRowsQuery q;
    q.rows = (int)v[0]; q.hq = (int)v[1]; q.hkv = (int)v[2]; q.head_dim = (int)v[3]; q.prefix_len = (int)v[4]; q.tail_len = (int)v[5];
    q.ldq = (long)v[6]; q.ldk = (long)v[7]; q.ldv = (long)v[8]; q.tail_ld = (long)v[9]; q.tail_row = (long)v[10];
    q.tail_slot_ld = (long)v[11]; q.has_slot = v[12] != 0; q.has_ws = v[13] != 0; q.nsplit = (int)v[14]; q.ws_bytes = (size_t)v[15];
    put(cogs_plan_attention_rows(q, tuning(tun)), out);
}
extern "C" int attn_nsplit(int ctx, const long long* tun) { return cogs_attn_nsplit(ctx, tuning(tun)); }
extern "C" int attn_rows_nsplit(int prefix_len, const long long* tun) { return cogs_attn_rows_nsplit(prefix_len, tuning(tun)); }
extern "C" long long attn_split_ws_bytes(int parts, int rows, int hq, int head_dim) {
    return (long long)cogs_attn_split_ws_bytes(parts, rows, hq, head_dim);
}
