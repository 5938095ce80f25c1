// Beam search on the device: the k best of rows x n candidate continuations, and the log-probabilities they are taken from.
//
// Replaces, per step of GenerationMixin._beam_search (transformers, reached from model/cogreasoner_chat.py:802-807 with
// num_beams > 1), `log_probs + running_beam_scores[:, :, None]` followed by torch.topk over the flattened [num_beams * vocab]
// row (_get_top_k_continuations): v(r, t) = scores[r][t] + row_add[r], the k largest in descending order, ties by ascending
// flat index r * n + t (torch.topk leaves the tie order open; here it is defined, so the same call gives the same result).
//
// Three launches at most, every score read once, integer LDS atomics only (they count and take maxima: the result does not
// depend on their order):
//   A  beam_slice_kernel   grid (slices, rows): a slice of one row (<= 4096 scores) goes to LDS as order-preserving keys and
//                          gives up its k best (key descending, flat index ascending), as sample_slice_topk_kernel does
//   B  beam_merge_kernel   grid (rows): the slices' lists of one row -> that row's k best
//   C  beam_merge_kernel   grid (1): the rows' lists -> the k best, written as (value, row, token)
// B is skipped while all of A's lists fit one merge (slices * rows <= 64). A merge first drops every candidate below T0 = the
// largest k-th key of any of its lists (that list alone holds k keys >= T0, so the k-th best overall is >= T0), then ranks
// the survivors against each other: rank = number of survivors in front, a total order, so every rank is taken once.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int BM_KMAX = 64;       // candidates per list
constexpr int BM_SLICE = 4096;    // scores per slice
constexpr int BM_SLICES = 64;     // slices per row
constexpr int BM_MERGE = 4096;    // candidates one merge holds: BM_SLICES lists of BM_KMAX

__device__ __forceinline__ uint32_t fkey(float s) {   // order-preserving float -> uint (never 0 for a non-NaN value)
    const uint32_t b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ bool better(uint32_t ka, int ia, uint32_t kb, int ib) {   // a before b (desc key, asc idx)
    return ka > kb || (ka == kb && ia < ib);
}

__global__ __launch_bounds__(256) void beam_slice_kernel(const float* __restrict__ scores, int n, long ld, const float* __restrict__ row_add,
                                                         int k, int chunk, uint32_t* __restrict__ cand_key, int* __restrict__ cand_idx) {
    __shared__ __attribute__((aligned(16))) uint32_t sl[BM_SLICE];
    __shared__ uint32_t wk[4];
    __shared__ int wi[4];
    const int row = blockIdx.y, lo = blockIdx.x * chunk, cnt = max(0, min(chunk, n - lo));      // lo, cnt: multiples of 4
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float add = row_add ? row_add[row] : 0.f;
    const float* src = scores + (long)row * ld + lo;
    for (int i = 4 * tid; i < cnt; i += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
        u32x4 key;
#pragma unroll
        for (int e = 0; e < 4; ++e) key[e] = fkey((v[e] + add) + 0.0f);      // + 0: a sum of -0 ranks as +0, as on the host
        *reinterpret_cast<u32x4*>(&sl[i]) = key;
    }
    __syncthreads();
    const long list = ((long)row * gridDim.x + blockIdx.x) * BM_KMAX;
    for (int r = 0; r < k; ++r) {
        uint32_t bk = 0u;
        int bi = 0x7fffffff;
        for (int i = tid; i < cnt; i += 256) {
            const uint32_t v = sl[i];
            if (better(v, i, bk, bi)) { bk = v; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t ok = __shfl_xor(bk, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (better(ok, oi, bk, bi)) { bk = ok; bi = oi; }
        }
        if (lane == 0) { wk[wid] = bk; wi[wid] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (better(wk[w], wi[w], bk, bi)) { bk = wk[w]; bi = wi[w]; }
            const bool ok = bk != 0u && bi < cnt;
            cand_key[list + r] = ok ? bk : 0u;                                // key 0 = "no candidate"
            cand_idx[list + r] = ok ? row * n + lo + bi : 0x7fffffff;
            if (ok) sl[bi] = 0u;
        }
        __syncthreads();
    }
}

// workgroup b merges lists [b * nlists, (b + 1) * nlists) -> list b of out_key / out_idx, or (out_val != null: the last merge)
// the k results themselves
__global__ __launch_bounds__(1024) void beam_merge_kernel(const uint32_t* __restrict__ in_key, const int* __restrict__ in_idx, int nlists,
                                                          int k, int n, uint32_t* __restrict__ out_key, int* __restrict__ out_idx,
                                                          float* __restrict__ out_val, int32_t* __restrict__ out_row,
                                                          int32_t* __restrict__ out_tok) {
    __shared__ __attribute__((aligned(16))) uint32_t ck[BM_MERGE];
    __shared__ __attribute__((aligned(16))) int ci[BM_MERGE];
    __shared__ uint32_t t0_sh;
    __shared__ int nsurv_sh;
    const int tid = threadIdx.x;
    const long base = (long)blockIdx.x * nlists * BM_KMAX;
    if (tid == 0) { t0_sh = 0u; nsurv_sh = 0; }
    __syncthreads();
    uint32_t kth = 0u;
    for (int l = tid; l < nlists; l += 1024) kth = max(kth, in_key[base + (long)l * BM_KMAX + k - 1]);
    if (kth) atomicMax(&t0_sh, kth);
    __syncthreads();
    const uint32_t T0 = t0_sh;
    for (int j = tid; j < nlists * k; j += 1024) {
        const long at = base + (long)(j / k) * BM_KMAX + j % k;
        const uint32_t key = in_key[at];
        if (key != 0u && key >= T0) {
            const int slot = atomicAdd(&nsurv_sh, 1);
            if (slot < BM_MERGE) { ck[slot] = key; ci[slot] = in_idx[at]; }
        }
    }
    __syncthreads();
    const int nsurv = min(nsurv_sh, BM_MERGE);
    const int nc = (nsurv + 3) & ~3;                                    // padded with "no candidate" entries
    if (tid < nc - nsurv) { ck[nsurv + tid] = 0u; ci[nsurv + tid] = 0x7fffffff; }
    __syncthreads();
    for (int j = tid; j < nsurv; j += 1024) {
        const uint32_t kj = ck[j];
        const int ij = ci[j];
        int rank = 0;
#pragma unroll 4
        for (int t = 0; t < nc; t += 4) {
            const u32x4 k4 = *reinterpret_cast<const u32x4*>(&ck[t]);
            const u32x4 i4 = *reinterpret_cast<const u32x4*>(&ci[t]);
#pragma unroll
            for (int e = 0; e < 4; ++e) rank += (k4[e] != 0u && better(k4[e], (int)i4[e], kj, ij)) ? 1 : 0;
        }
        if (rank >= k) continue;
        if (out_val) {
            out_val[rank] = fkey_inv(kj);
            out_row[rank] = ij / n;
            out_tok[rank] = ij % n;
        } else {
            out_key[(long)blockIdx.x * BM_KMAX + rank] = kj;
            out_idx[(long)blockIdx.x * BM_KMAX + rank] = ij;
        }
    }
    if (!out_val && tid >= nsurv && tid < k) {                          // fewer candidates than k: the rest of the list is empty
        out_key[(long)blockIdx.x * BM_KMAX + tid] = 0u;
        out_idx[(long)blockIdx.x * BM_KMAX + tid] = 0x7fffffff;
    }
}

__global__ __launch_bounds__(256) void sub_rows_kernel(float* __restrict__ x, int n, long ld, const float* __restrict__ sub) {
    const float s = sub[blockIdx.y];
    float* row = x + (long)blockIdx.y * ld;
    for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < n; i += 4 * 256 * gridDim.x) {
        f32x4 v = *reinterpret_cast<f32x4*>(row + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] -= s;
        *reinterpret_cast<f32x4*>(row + i) = v;
    }
}

struct BeamPlan { int nslice, chunk; bool two_level; };
BeamPlan beam_plan(int rows, int n) {
    BeamPlan p;
    p.nslice = n / 1024 < 1 ? 1 : (n / 1024 > BM_SLICES ? BM_SLICES : n / 1024);
    p.chunk = (((n + p.nslice - 1) / p.nslice) + 3) & ~3;
    p.two_level = p.nslice * rows > BM_SLICES;
    return p;
}

}  // namespace

static int beam_args_ok(int rows, int n, int k) {
    if (rows < 1 || n < 1 || k < 1 || (n & 3) || (long)k > (long)rows * n) return COGS_E_INVALID;
    if (rows > 16 || k > BM_KMAX || n > BM_SLICES * BM_SLICE) return COGS_E_UNSUPPORTED;
    return COGS_OK;
}

int cogs_k_beam_topk_ws(int rows, int n, int k, size_t* bytes) {
    const int rc = beam_args_ok(rows, n, k);
    if (rc != COGS_OK) return rc;
    const BeamPlan p = beam_plan(rows, n);
    *bytes = ((size_t)rows * p.nslice + (p.two_level ? rows : 0)) * BM_KMAX * 8;
    return COGS_OK;
}

int cogs_k_beam_topk(hipStream_t st, const float* scores, int rows, int n, long ld, const float* row_add, int k, float* out_val,
                     int32_t* out_row, int32_t* out_tok, void* ws, size_t ws_bytes) {
    const int rc = beam_args_ok(rows, n, k);
    if (rc != COGS_OK) return rc;
    if (!scores || !out_val || !out_row || !out_tok || ld < n || (ld & 3) || ((uintptr_t)scores & 15)) return COGS_E_INVALID;
    const BeamPlan p = beam_plan(rows, n);
    const size_t lists = (size_t)rows * p.nslice, lists2 = p.two_level ? rows : 0;
    if (!ws || ws_bytes < (lists + lists2) * BM_KMAX * 8) return COGS_E_WORKSPACE;
    uint32_t* key_a = (uint32_t*)ws;
    int* idx_a = (int*)(key_a + lists * BM_KMAX);
    uint32_t* key_b = (uint32_t*)(idx_a + lists * BM_KMAX);
    int* idx_b = (int*)(key_b + lists2 * BM_KMAX);
    hipLaunchKernelGGL(beam_slice_kernel, dim3(p.nslice, rows), dim3(256), 0, st, scores, n, ld, row_add, k, p.chunk, key_a, idx_a);
    if (p.two_level) {
        hipLaunchKernelGGL(beam_merge_kernel, dim3(rows), dim3(1024), 0, st, key_a, idx_a, p.nslice, k, n, key_b, idx_b, (float*)nullptr,
                           (int32_t*)nullptr, (int32_t*)nullptr);
        hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(1024), 0, st, key_b, idx_b, rows, k, n, (uint32_t*)nullptr, (int*)nullptr,
                           out_val, out_row, out_tok);
    } else {
        hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(1024), 0, st, key_a, idx_a, p.nslice * rows, k, n, (uint32_t*)nullptr,
                           (int*)nullptr, out_val, out_row, out_tok);
    }
    return COGS_LAUNCH_CHECK();
}

// x[r][i] -= sub[r]: logits -> log-probabilities with sub = the rows' log-sum-exp (cogs_row_lse)
int cogs_k_sub_rows(hipStream_t st, float* x, int rows, int n, long ld, const float* sub) {
    if (!x || !sub || rows < 1 || n < 1 || (n & 3) || ld < n || (ld & 3) || ((uintptr_t)x & 15)) return COGS_E_INVALID;
    const int bx = (n / 4 + 255) / 256;
    hipLaunchKernelGGL(sub_rows_kernel, dim3(bx > 64 ? 64 : bx, rows), dim3(256), 0, st, x, n, ld, sub);
    return COGS_LAUNCH_CHECK();
}
