// Teacher-forced scoring: per-row log-sum-exp / target logit / first-maximum argmax of a logits matrix that is never
// materialised as a whole. The caller (capi_llm.hip: cogs_lm_score, capi.hip: cogs_row_lse) walks row blocks x vocabulary panels; a
// panel [rows_b, width] of fp32 logits is folded into per-row running state (max, sum of exp relative to the max,
// argmax) by the online-softmax update, and a last kernel turns the state into lse = max + log(sum).
//
// Replaces (third-party, transformers as pinned by the reference): Qwen2ForCausalLM.forward's
//   logits = lm_head(hidden_states).float(); ForCausalLMLoss -> F.cross_entropy(shift_logits, shift_labels,
//   ignore_index=-100)
// behind model/cogreasoner_chat.py:680-693 (forward_train) and :737-751 (forward), which builds the [S, vocab] fp32
// logits (2.5 GB for a 4 096-token prompt at vocab 152 064) to read one number per row out of them.
//
// lse_fold_kernel is the hot path: one workgroup per (row, column chunk), every panel line read exactly once with 16-byte
// loads (16 values per thread in flight), per-thread online update with ONE rescale per 16 values, exp2 on differences
// scaled by log2(e), wave reduction by DPP (common.h), LDS only to join the four waves. With few rows the columns of a
// panel are split over workgroups (partials merged in column order by lse_merge_kernel, as attn_decode + combine and
// argmax_part + argmax_final do). Every merge has a fixed order and uses no floating-point atomics: results are
// bit-reproducible run to run.
#include "common.h"
#include "kernels.h"
#include "debug.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int NO_IDX = 0x7fffffff;
constexpr int FOLD_THREADS = 256;
constexpr int FOLD_UNROLL = 4;          // 16-byte loads in flight per thread
constexpr size_t PANEL_BYTES = 64u << 20;   // design condition of cogs_lm_score (include/cogs.h)

struct __attribute__((aligned(16))) LseState {
    float mx;    // maximum so far (exact)
    float l;     // sum of exp(x - mx) so far
    int bi;      // column of the first maximum (NO_IDX: none yet)
    int pad;
};

// exp(a - b) for a <= b; a == -inf (nothing seen yet, or a row of -inf) contributes nothing
__device__ __forceinline__ float exp_diff(float a, float b) {
    return a == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((a - b) * LOG2E);
}
// a covers earlier columns than b
__device__ __forceinline__ LseState lse_merge(const LseState& a, const LseState& b) {
    LseState r;
    r.mx = fmaxf(a.mx, b.mx);
    r.l = a.l * exp_diff(a.mx, r.mx) + b.l * exp_diff(b.mx, r.mx);
    r.bi = b.mx > a.mx ? b.bi : (b.mx == a.mx ? min(a.bi, b.bi) : a.bi);
    r.pad = 0;
    return r;
}
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// grid (rows, nsplit). panel: fp32 [rows][ld], 16-byte aligned rows; this workgroup folds columns [s * chunk,
// min(width, (s + 1) * chunk)) of row r (chunk % 32 == 0: whole 128-byte lines). col0 = vocabulary column of panel
// column 0. DIRECT (nsplit == 1): the result is merged into state[r] right here (first != 0: state[r] is not read);
// else it goes to part[r * nsplit + s] for lse_merge_kernel.
template <bool DIRECT>
__global__ __launch_bounds__(FOLD_THREADS) void lse_fold_kernel(const float* __restrict__ panel, long ld, int width, int col0,
                                                                int chunk, int first, const int64_t* __restrict__ targets,
                                                                float* __restrict__ target_logit, LseState* __restrict__ state,
                                                                LseState* __restrict__ part) {
    __shared__ LseState sw[FOLD_THREADS / 64];
    const int r = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int c_lo = s * chunk, c_hi = min(width, c_lo + chunk);
    const float* __restrict__ row = panel + (long)r * ld;
    const int n4 = (c_hi - c_lo) >> 2;
    const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(row + c_lo);

    float mx = -INFINITY, l = 0.f;
    int bi = NO_IDX;
    for (int i = tid; i < n4; i += FOLD_THREADS * FOLD_UNROLL) {
        f32x4 v[FOLD_UNROLL];
#pragma unroll
        for (int j = 0; j < FOLD_UNROLL; ++j) {
            const int k = i + j * FOLD_THREADS;
            const f32x4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            v[j] = k < n4 ? p4[k] : ninf;
        }
        // maximum of the 16 values and its first column (ascending columns, strict >)
        float cm = -INFINITY;
        int ci = NO_IDX;
#pragma unroll
        for (int j = 0; j < FOLD_UNROLL; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (v[j][e] > cm) { cm = v[j][e]; ci = c_lo + ((i + j * FOLD_THREADS) << 2) + e; }
        if (cm > mx) {      // the row maximum (as seen by this thread) moves: one rescale for the 16 values
            l *= exp_diff(mx, cm);
            mx = cm; bi = ci;
        }
        const float base = mx == -INFINITY ? 0.f : mx;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < FOLD_UNROLL; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += __builtin_amdgcn_exp2f((v[j][e] - base) * LOG2E);
        l += acc;
    }
    // wave: common maximum, rescaled sums, lowest column among the lanes that hold the maximum
    const float wm = wave_max(mx);
    const float wl = wave_sum(l * exp_diff(mx, wm));
    const int wi = wave_min_int(mx == wm ? bi : NO_IDX);
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) { sw[wid].mx = wm; sw[wid].l = wl; sw[wid].bi = wi; sw[wid].pad = 0; }
    __syncthreads();
    if (tid == 0) {
        // the waves interleave columns: the merge is order-free in value (max / sum / min index), fixed in sequence
        LseState a = sw[0];
#pragma unroll
        for (int w = 1; w < FOLD_THREADS / 64; ++w) a = lse_merge(a, sw[w]);
        if (a.bi != NO_IDX) a.bi += col0;
        if constexpr (DIRECT) {
            state[r] = first ? a : lse_merge(state[r], a);
        } else {
            part[(long)r * gridDim.y + s] = a;
        }
        if (target_logit && targets) {   // exactly one workgroup of the whole walk owns a row's target column
            const int64_t t = targets[r] - col0;
            if (t >= c_lo && t < c_hi) target_logit[r] = row[t];
        }
    }
}

// one thread per row: partials of one panel in column order, behind the running state
__global__ __launch_bounds__(256) void lse_merge_kernel(const LseState* __restrict__ part, int nsplit, int rows, int first,
                                                        LseState* __restrict__ state) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const LseState* p = part + (long)r * nsplit;
    LseState a = p[0];
    for (int s = 1; s < nsplit; ++s) a = lse_merge(a, p[s]);
    state[r] = first ? a : lse_merge(state[r], a);
}

__global__ __launch_bounds__(256) void lse_final_kernel(const LseState* __restrict__ state, int rows, int n,
                                                        const int64_t* __restrict__ targets, float* __restrict__ lse,
                                                        float* __restrict__ target_logit, int64_t* __restrict__ argmax,
                                                        float* __restrict__ max_logit, int* __restrict__ n_bad) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const LseState a = state[r];
    if (lse) lse[r] = a.mx == -INFINITY ? -INFINITY : a.mx + logf(a.l);
    if (max_logit) max_logit[r] = a.mx;
    if (argmax) argmax[r] = a.bi == NO_IDX ? 0 : a.bi;
    const int64_t t = targets ? targets[r] : -100;
    if (t < 0 || t >= n) {       // ignored row (-100), or a target outside the vocabulary: ignored and counted
        if (target_logit) target_logit[r] = 0.f;
        if (t != -100 && n_bad) atomicAdd(n_bad, 1);      // integer count: order-free
    }
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace

// Geometry of the walk over a [rows, n] logits matrix: rows_b x cols_p panels, chunk columns per workgroup of the fold.
// The panel never exceeds 64 MiB, whatever the switches say.
void cogs_k_lse_plan(int rows, int n, CogsLsePlan* p) {
    const long long sw_rows = g_cogs_debug.lm_score_rows, sw_cols = g_cogs_debug.lm_score_cols, sw_split = g_cogs_debug.lm_score_split;
    int rows_b = (int)(sw_rows < rows ? sw_rows : rows);
    if (rows_b < 1) rows_b = 1;
    const long long fit = (long long)(PANEL_BYTES / sizeof(float)) / rows_b;     // columns of a 64 MiB panel
    long long cols = sw_cols > 0 ? sw_cols : fit;
    if (cols > fit) cols = fit;
    int cols_p;
    if (cols >= n) cols_p = n;
    else { cols_p = (int)(cols / 32 * 32); if (cols_p < 32) cols_p = 32; }
    int nsplit;
    if (sw_split > 0) nsplit = (int)sw_split;
    else nsplit = rows_b >= 512 ? 1 : (1024 + rows_b - 1) / rows_b;      // about 1024 workgroups: four per CU
    int chunk = round_up((cols_p + nsplit - 1) / nsplit, 32);
    if (sw_split <= 0 && chunk < 1024) chunk = 1024;                      // at least one 16-byte load per thread
    nsplit = (cols_p + chunk - 1) / chunk;
    p->rows_b = rows_b; p->cols_p = cols_p; p->chunk = chunk; p->nsplit = nsplit;
    p->state_bytes = (size_t)rows * sizeof(LseState);
    p->part_bytes = nsplit > 1 ? (size_t)rows_b * nsplit * sizeof(LseState) : 0;
    p->panel_bytes = (size_t)rows_b * cols_p * sizeof(float);
}

int cogs_k_lse_fold(hipStream_t st, const CogsLsePlan& p, const float* panel, long ld, int rows, int width, int col0,
                    const int64_t* targets, float* target_logit, void* state, void* part) {
    if (rows <= 0 || width <= 0 || rows > p.rows_b || width > p.cols_p) return COGS_E_INVALID;
    if ((width & 3) || (ld & 3) || ((uintptr_t)panel & 15)) return COGS_E_INVALID;
    const int nsplit = (width + p.chunk - 1) / p.chunk;
    const int first = col0 == 0;
    if (nsplit == 1) {
        hipLaunchKernelGGL(lse_fold_kernel<true>, dim3(rows, 1), dim3(FOLD_THREADS), 0, st, panel, ld, width, col0, p.chunk, first,
                           targets, target_logit, (LseState*)state, (LseState*)nullptr);
    } else {
        if (!part) return COGS_E_WORKSPACE;
        hipLaunchKernelGGL(lse_fold_kernel<false>, dim3(rows, nsplit), dim3(FOLD_THREADS), 0, st, panel, ld, width, col0, p.chunk,
                           first, targets, target_logit, (LseState*)state, (LseState*)part);
        hipLaunchKernelGGL(lse_merge_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, (const LseState*)part, nsplit, rows,
                           first, (LseState*)state);
    }
    return COGS_LAUNCH_CHECK();
}

int cogs_k_lse_final(hipStream_t st, const void* state, int rows, int n, const int64_t* targets, float* lse,
                     float* target_logit, int64_t* argmax, float* max_logit, int* n_bad) {
    if (rows <= 0) return COGS_E_INVALID;
    if (n_bad && hipMemsetAsync(n_bad, 0, sizeof(int), st) != hipSuccess) return COGS_E_HIP;
    hipLaunchKernelGGL(lse_final_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, (const LseState*)state, rows, n, targets, lse,
                       target_logit, argmax, max_logit, n_bad);
    return COGS_LAUNCH_CHECK();
}
