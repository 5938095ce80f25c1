// Single-token (decode) attention, key-split: bf16, head dim 128, pre-scaled Q, GQA with up to 16 query heads per
// key/value head packed into the 16 query columns of one MFMA tile.
//
// Replaces, for the generated tokens, the attention inside Qwen2Model.forward (transformers 4.46.3, reached from
// model/cogreasoner_chat.py:802 through GenerationMixin): one new query row against the whole KV cache. HBM-bound:
// the step streams 57 344 B x context per layer once (31.5 MB at 15.4k tokens).
//
// The general kernel (attn.hip, gqa_pack mode) walks the 64-key tiles of a split one after the other with ONE wave
// computing and all four staging: per tile load -> barrier -> LDS write -> barrier -> compute, four dependent rounds of
// ~1.5 us per 256-key split and 32 KiB in flight per CU (13.5 us per layer, 2.3 TB/s). Here every WAVE owns whole tiles
// (tile t of a split goes to wave t & 3): it requests its K and V tile at once (32 non-temporal 16-byte loads per
// lane: 128 KiB in flight per CU), takes K straight into MFMA A fragments (no LDS), passes V through a wave-private
// LDS region for the transposing fragment reads (no workgroup barrier), runs S^T = K.Q^T -> softmax -> O^T = V^T.P^T on
// its own, and the four waves' (m, l, O) are merged through LDS into the split's partial -- the same partial format as
// before, so attn.hip's combine kernel is reused unchanged.
//
// v_mfma_f32_16x16x32_bf16, S^T[key][q]: lane (li = lane & 15, g = lane >> 4) of the accumulator of key block u holds
// keys 16u + 4g + r (r = register) of query column li; those registers of blocks 2c, 2c+1 ARE the B operand of k-step c
// of O^T (k-slot 8g + e <-> key 32c + 16(e >> 2) + 4g + (e & 3)), and the matching V^T A fragment is two
// ds_read_b64_tr_b16 (keys 32c + 4g + 0..3 and + 16) of the row-major V tile. V rows are 288 B apart in LDS: the 8 rows a
// transposing read touches per cycle start in 8 different 32-byte bank groups.
#include "common.h"
#include "kernels.h"

namespace {

struct DecodeAttnArgs {
    const bf16_t* Q; const bf16_t* K; const bf16_t* V;
    long ldk, ldv;                 // elements
    int kend;                      // keys 0 .. kend-1 are visible
    int hq, hkv, nsplit, gsz;
    float* part_o;                 // [nsplit][hq][128] unnormalised, relative to part_ml[..][0]
    float* part_ml;                // [nsplit][hq][2] (running max in log2 units, sum)
    // multi-row form (ROWS): `rows` query rows share keys [0, kend) of K / V and own keys [0, tail_len) of tail_k / tail_v[row]
    const bf16_t* tail_k; const bf16_t* tail_v;
    long ldq, tail_ld, tail_row;   // elements: Q row stride, tail key stride, tail stride between rows
    int rows, ntile, tail_len;     // ntile = ceil(rows * gsz / 16) column tiles per kv head
    // SLOT: key j of row r's tail is read from tail slot tail_slot[r * tail_slot_ld + j] (beam search: a row continues another
    // row's tail without copying it)
    const int* tail_slot; long tail_slot_ld;
};

// max / sum over the four lanes {li, li+16, li+32, li+48} (one query column), result in all four (see attn.hip)
__device__ __forceinline__ float col_max4(float x) {
    const unsigned xb = __builtin_bit_cast(unsigned, x);
    const auto a = __builtin_amdgcn_permlane16_swap(xb, xb, false, false);
    const float y = fmaxf(__builtin_bit_cast(float, (unsigned)a[0]), __builtin_bit_cast(float, (unsigned)a[1]));
    const unsigned yb = __builtin_bit_cast(unsigned, y);
    const auto b = __builtin_amdgcn_permlane32_swap(yb, yb, false, false);
    return fmaxf(__builtin_bit_cast(float, (unsigned)b[0]), __builtin_bit_cast(float, (unsigned)b[1]));
}
__device__ __forceinline__ float col_sum4(float x) {
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    return x;
}

// ROWS (cogs_attention_rows): the rows * gsz query columns of a kv head are packed into ntile tiles of 16 -- column c is head
// c % gsz of row c / gsz, a row's heads may straddle two tiles -- and workgroup x < nsplit * ntile runs split x % nsplit of
// the shared keys for tile x / nsplit; workgroup nsplit * ntile + r runs row r's own tail as ONE more partial (index nsplit)
// of that row's gsz columns. Partials are [nsplit + 1][rows * hq] slots: the combine kernel sees rows * hq heads.
// SLOT (ROWS only): the tail workgroup forms every key row's address from the row's slot table -- key j at slot s[j] * tail_row +
// j * tail_ld -- where it otherwise adds one row base; an entry outside [0, rows) is clamped (it then reads some row's tail, never
// outside the buffers). The shared-prefix workgroups are the ROWS ones.
template <bool ROWS, bool SLOT = false>
__global__ __launch_bounds__(256, 1) void attn_decode_kernel(DecodeAttnArgs p) {
    constexpr int HD = 128, VRS = 288, VT = 64 * VRS;
    __shared__ __attribute__((aligned(16))) char vs[4 * VT];          // one V tile per wave
    __shared__ float cm[4][16], cl[4][16];
    __shared__ float co[4][16][HD + 4];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int kvh = blockIdx.y;
    const int gsz = p.gsz;                                       // hq / hkv, divided on the host
    int split = blockIdx.x, nsplit = p.nsplit, kend = p.kend, ncols = gsz, part = blockIdx.x;
    const bf16_t* Kp = p.K; const bf16_t* Vp = p.V;
    long ldk = p.ldk, ldv = p.ldv;
    long qoff = (long)(kvh * gsz + li) * HD;                     // this lane's query column: element offset in Q ...
    int oslot = kvh * gsz + li;                                  // ... and its (row, head) slot inside one partial
    const int* srow = nullptr;                                   // SLOT, tail workgroup: this row's slot table
    if constexpr (ROWS) {
        const int shared_blocks = p.nsplit * p.ntile;
        if ((int)blockIdx.x < shared_blocks) {
            split = blockIdx.x % p.nsplit; part = split;
            const int c0 = 16 * (int)(blockIdx.x / p.nsplit);
            ncols = min(16, p.rows * gsz - c0);
            const int row = (c0 + li) / gsz, hh = (c0 + li) - row * gsz;
            qoff = (long)row * p.ldq + (long)(kvh * gsz + hh) * HD;
            oslot = row * p.hq + kvh * gsz + hh;
        } else {
            const int row = blockIdx.x - shared_blocks;
            split = 0; nsplit = 1; part = p.nsplit; kend = p.tail_len;
            if constexpr (SLOT) { Kp = p.tail_k; Vp = p.tail_v; srow = p.tail_slot + (long)row * p.tail_slot_ld; }
            else { Kp = p.tail_k + (long)row * p.tail_row; Vp = p.tail_v + (long)row * p.tail_row; }
            ldk = ldv = p.tail_ld;
            qoff = (long)row * p.ldq + (long)(kvh * gsz + li) * HD;
            oslot = row * p.hq + kvh * gsz + li;
        }
    }

    // (unsigned 32-bit: tiles x splits is far below 2^32, checked by the launcher; the signed 64-bit form was two ~100-instruction
    // divisions at the head of a 10 us kernel)
    const unsigned nt_all = (unsigned)(kend + 63) >> 6;
    const int t_begin = (int)(nt_all * (unsigned)split / (unsigned)nsplit);
    const int t_end = (int)(nt_all * (unsigned)(split + 1) / (unsigned)nsplit);

    // Q fragments (B operand of S^T = K.Q^T): lane (q = li, g) holds Q[head kvh*gsz + li][32s + 8g .. +7]
    bf16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        u32x4 v = {0, 0, 0, 0};
        if (li < ncols) v = *reinterpret_cast<const u32x4*>(p.Q + qoff + 32 * s + 8 * g);
        qf[s] = __builtin_bit_cast(bf16x8, v);
    }

    f32x4 oacc[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) oacc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;      // running maximum of the column (same in its four lanes), this lane's share of the sum

    char* const vw = vs + wid * VT;
    const int v_wr = (lane >> 4) * VRS + (lane & 15) * 16;                         // + 4i rows: row (lane>>4) + 4i, chunk lane&15
    const int v_rd = (4 * g + (li >> 2)) * VRS + (li & 3) * 8;                     // + (32c [+16]) rows + 32 db bytes

    for (int kt = t_begin + wid; kt < t_end; kt += 4) {
        const int kbase = kt * 64;
        const int nvalid = min(64, kend - kbase);                                  // >= 1
        const bf16_t* kb = Kp + (long)kbase * ldk + kvh * HD;
        const bf16_t* vb = Vp + (long)kbase * ldv + kvh * HD;
        // every byte is read once per token by this wave: non-temporal. Rows past the end repeat the last row
        // (finite data; their scores are masked)
        u32x4 kf[4][4], vreg[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kr = min(16 * u + li, nvalid - 1);
            long ro = (long)kr * ldk;
            if constexpr (SLOT) { if (srow) ro += (long)min(max(srow[kbase + kr], 0), p.rows - 1) * p.tail_row; }
#pragma unroll
            for (int s = 0; s < 4; ++s)
                kf[u][s] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + ro + 32 * s + 8 * g));
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kr = min((lane >> 4) + 4 * i, nvalid - 1);
            long ro = (long)kr * ldv;
            if constexpr (SLOT) { if (srow) ro += (long)min(max(srow[kbase + kr], 0), p.rows - 1) * p.tail_row; }
            vreg[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vb + ro + (lane & 15) * 8));
        }
        // S^T, four key blocks of 16
        f32x4 sacc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sacc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s)
                sacc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[u][s]), qf[s], sacc[u], 0, 0, 0);
        }
        // V tile -> this wave's LDS region (the previous tile's fragment reads of this wave are complete: in-order LDS)
#pragma unroll
        for (int i = 0; i < 16; ++i) *reinterpret_cast<u32x4*>(vw + v_wr + 4 * i * VRS) = vreg[i];
        // softmax of the tile (scores are in log2 units: Q is pre-scaled)
        float tmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (16 * u + 4 * g + r >= nvalid) sacc[u][r] = -INFINITY;
                tmax = fmaxf(tmax, sacc[u][r]);
            }
        tmax = col_max4(tmax);                                   // finite: key kbase exists
        const float m_new = fmaxf(m, tmax);
        const float alpha = (m == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m - m_new);
        float psum = 0.f;
        bf16x8 pf[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            u32x4 w;
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) {
                const int e = 2 * e2;
                const float p0 = __builtin_amdgcn_exp2f(sacc[2 * c + (e >> 2)][e & 3] - m_new);
                const float p1 = __builtin_amdgcn_exp2f(sacc[2 * c + ((e + 1) >> 2)][(e + 1) & 3] - m_new);
                psum += p0 + p1;
                w[e2] = pack_bf2(p0, p1);
            }
            pf[c] = __builtin_bit_cast(bf16x8, w);
        }
        l = l * alpha + psum;
        m = m_new;
#pragma unroll
        for (int db = 0; db < 8; ++db) oacc[db] *= alpha;
        // O^T += V^T . P^T
#pragma unroll
        for (int db = 0; db < 8; ++db)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const char* va = vw + v_rd + 32 * c * VRS + 32 * db;
                const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(va));
                const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(va + 16 * VRS));
                const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
                const u32x4 a = u32x4{l2[0], l2[1], h2[0], h2[1]};
                oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), pf[c], oacc[db], 0, 0, 0);
            }
    }

    // merge the four waves: (m, l, O) per query column through LDS
    l = col_sum4(l);
    if (g == 0) { cm[wid][li] = m; cl[wid][li] = l; }
    __shared__ int cslot[16];
    if constexpr (ROWS) { if (lane == li && wid == 0) cslot[li] = oslot; }
    if (li < ncols) {
#pragma unroll
        for (int db = 0; db < 8; ++db) *reinterpret_cast<f32x4*>(&co[wid][li][16 * db + 4 * g]) = oacc[db];
    }
    __syncthreads();
    for (int idx = tid; idx < ncols * HD; idx += 256) {
        const int q = idx / HD, d = idx % HD;
        const float M = fmaxf(fmaxf(cm[0][q], cm[1][q]), fmaxf(cm[2][q], cm[3][q]));
        float o = 0.f, L = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float wt = (cm[w][q] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(cm[w][q] - M);
            o += co[w][q][d] * wt;
            L += cl[w][q] * wt;
        }
        long slot = (long)split * p.hq + kvh * gsz + q;
        if constexpr (ROWS) slot = (long)part * p.rows * p.hq + cslot[q];
        p.part_o[slot * HD + d] = (M == -INFINITY) ? 0.f : o;
        if (d == 0) { p.part_ml[slot * 2] = M; p.part_ml[slot * 2 + 1] = L; }
    }
}

}  // namespace

// single query row, bf16, hd 128, pre-scaled Q, keys split over plan.nsplit workgroups per kv head; partials in the
// layout attn.hip's attn_combine_kernel reads (q_len = 1). Validation, key count and grid: cogs_plan_attention (attn_plan.h)
int cogs_k_attention_decode(hipStream_t st, const CogsAttn& a, const AttnPlan& plan, float* part_o, float* part_ml) {
    DecodeAttnArgs p;
    p.Q = (const bf16_t*)a.Q; p.K = (const bf16_t*)a.K; p.V = (const bf16_t*)a.V;
    p.ldk = a.ldk; p.ldv = a.ldv;
    p.kend = plan.kend;
    p.hq = a.hq; p.hkv = a.hkv; p.nsplit = plan.nsplit; p.gsz = plan.gsz;
    p.part_o = part_o; p.part_ml = part_ml;
    p.tail_k = p.tail_v = nullptr; p.ldq = p.tail_ld = p.tail_row = 0; p.rows = 1; p.ntile = 1; p.tail_len = 0;
    p.tail_slot = nullptr; p.tail_slot_ld = 0;
    hipLaunchKernelGGL(attn_decode_kernel<false>, dim3(plan.grid_x, plan.grid_y), dim3(plan.block_x), 0, st, p);
    return COGS_LAUNCH_CHECK();
}

// `rows` query rows in lockstep over one shared prompt (cogs_attention_rows, include/cogs.h): key-split partials of the shared
// keys + one partial per row for its own tail, part_o / part_ml sized for plan.parts partials of rows * hq heads
// (cogs_plan_attention_rows)
int cogs_k_attention_decode_rows(hipStream_t st, const CogsAttnRows& a, const AttnPlan& plan, float* part_o, float* part_ml) {
    DecodeAttnArgs p;
    p.Q = (const bf16_t*)a.Q; p.K = (const bf16_t*)a.K; p.V = (const bf16_t*)a.V;
    p.ldk = a.ldk; p.ldv = a.ldv;
    p.kend = plan.kend;
    p.hq = a.hq; p.hkv = a.hkv; p.nsplit = plan.nsplit; p.gsz = plan.gsz;
    p.part_o = part_o; p.part_ml = part_ml;
    p.tail_k = (const bf16_t*)a.tail_k; p.tail_v = (const bf16_t*)a.tail_v;
    p.ldq = a.ldq; p.tail_ld = a.tail_ld; p.tail_row = a.tail_row;
    p.rows = a.rows; p.ntile = plan.ntile; p.tail_len = a.tail_len;
    p.tail_slot = a.tail_slot; p.tail_slot_ld = a.tail_slot_ld;
    const dim3 grid(plan.grid_x, plan.grid_y), block(plan.block_x);
    if (plan.rows_slot) hipLaunchKernelGGL((attn_decode_kernel<true, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL(attn_decode_kernel<true>, grid, block, 0, st, p);
    return COGS_LAUNCH_CHECK();
}
