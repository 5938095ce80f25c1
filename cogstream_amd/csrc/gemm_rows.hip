// Multi-row weight-streaming GEMM for lockstep decode:  C[M,N] = epilogue( A[M,K] . W[N,K]^T ), bf16, 1 <= M <= 16.
//
// The step that advances several sampled continuations of one prompt (cogs_llm_decode_rows; the reference reaches the
// same arithmetic through GenerationMixin.generate(num_return_sequences=N), model/cogreasoner_chat.py:802-807) is bound
// by the weight bytes exactly like the single-row GEMV (gemv.hip), but the GEMV's products run on the vector ALU: 8
// instructions per 16 weight bytes and per ROW of activations. Here the weights are the streamed operand of
// v_mfma_f32_16x16x32_bf16 and the M activation rows are its 16 columns (columns >= M are zero): one instruction
// multiplies 1 KiB of weights with up to 16 rows, and every weight byte is read once per step, not once per sequence.
//
// One wave owns a block of 16 output columns (16 weight rows). Per 64-element k-chunk lane (r = lane & 15, g = lane >> 4)
// loads the 32 contiguous bytes k = 64c + 16g .. + 15 of weight row r (two 16-byte non-temporal loads, straight to
// registers: nothing is shared between waves, an LDS round trip would be pure overhead); the four lane groups of a
// row together read one whole 128-byte line. The two loads are the A fragments of two MFMAs: MFMA h of the chunk takes
// fragment element j of lane group g from k = 64c + 16g + 8h + j. The sum over k does not care about the order as
// long as both operands agree, so the activation fragment of lane (m = lane & 15, g) is read at the same k (32 contiguous
// bytes of row m, from L2: the activations are at most 16 x K x 2 bytes and every wave re-reads them). U chunks are
// requested per batch and the next batch is requested before the current one is multiplied (late waits).
//
// Small N (o / down: 224 column blocks on 256 CUs): the KS waves of a workgroup split the k-chunks of ONE column block
// (chunk c goes to wave c % KS), park their accumulators in LDS and wave 0 adds them in wave order. No floating-point
// atomics: the same call gives the same bits. MFMA columns never mix and the split depends on N and K only, so output
// row m does not depend on the other rows or on the slot it sits in.
//
// Accumulator layout (cdna guide, section 3): lane (m = lane & 15, g) holds columns n0 + 4g .. + 3 of row m -- the four
// consecutive columns epilogue4() expects (bias / rotary pairs / SwiGLU pairs / residual / fp32 output).
#include "common.h"
#include "kernels.h"
#include "gemm_epilogue.h"

namespace {

struct RowsArgs {
    const bf16_t* A; long lda;     // elements
    const bf16_t* W; long ldw;
    int M, N, K;
    EpiArgs epi;
};

// KS: waves that share one column block's k range (1: every wave of the workgroup has its own blocks);
// CB: column blocks of 16 per wave (they share the activation fragments); U: k-chunks per batch
template <int KS, int CB, int U>
__global__ __launch_bounds__(KS == 1 ? 256 : 64 * KS) void gemm_rows_kernel(RowsArgs p) {
    constexpr int NW = KS == 1 ? 4 : KS;
    __shared__ f32x4 red[KS > 1 ? KS : 1][CB][64];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int n0 = (KS == 1 ? blockIdx.x * NW + wid : blockIdx.x) * 16 * CB;
    if (KS == 1 && n0 >= p.N) return;               // whole waves, and this form has no barrier
    const int ks = KS == 1 ? 0 : wid;
    const int nch = p.K >> 6;

    // rows past the end of W repeat the last row (finite data; their columns are never stored)
    const bf16_t* wp[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) wp[cb] = p.W + (long)min(n0 + 16 * cb + r, p.N - 1) * p.ldw + 16 * g;
    const bool a_on = r < p.M;
    const bf16_t* ap = p.A + (long)min(r, p.M - 1) * p.lda + 16 * g;

    struct Batch { u32x4 w[U][CB][2]; u32x4 a[U][2]; };
    auto load = [&](Batch& b, int c0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * KS;              // wave-uniform
            if (c < nch) {
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        b.w[u][cb][h] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[cb] + c * 64 + 8 * h));
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    b.a[u][h] = u32x4{0, 0, 0, 0};
                    if (a_on) b.a[u][h] = *reinterpret_cast<const u32x4*>(ap + c * 64 + 8 * h);
                }
            } else {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) b.w[u][cb][h] = u32x4{0, 0, 0, 0};
                    b.a[u][h] = u32x4{0, 0, 0, 0};
                }
            }
        }
    };

    f32x4 acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    Batch cur;
    load(cur, ks);
    for (int c = ks; c < nch; c += U * KS) {
        Batch nxt;
        load(nxt, c + U * KS);                      // past the end: zeros, no memory access
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u * KS >= nch) continue;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cur.w[u][cb][h]),
                                                                      __builtin_bit_cast(bf16x8, cur.a[u][h]), acc[cb], 0, 0, 0);
        }
        cur = nxt;
    }

    if constexpr (KS > 1) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) red[wid][cb][lane] = acc[cb];
        __syncthreads();
        if (wid != 0) return;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            f32x4 s = red[0][cb][lane];
#pragma unroll
            for (int w = 1; w < KS; ++w) s += red[w][cb][lane];
            acc[cb] = s;
        }
    }
    if (!a_on) return;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int n = n0 + 16 * cb + 4 * g;         // N % 4 == 0: a lane's four columns are inside or outside together
        if (n < p.N) epilogue4<bf16_t>(p.epi, r, n, acc[cb]);
    }
}

}  // namespace

int cogs_k_gemm_rows(hipStream_t st, const CogsGemm& g) {
    if (g.dtype != COGS_DT_BF16 || g.M > 16) return COGS_E_UNSUPPORTED;
    if (g.ln_ab || g.row_stats || g.hm_rows > 0 || g.rope_lut || g.rms_gamma || g.kv_k ||
        g.act == COGS_ACT_GELU_TANH || g.act == COGS_ACT_GELU_ERF)
        return COGS_E_UNSUPPORTED;
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.K % 64 != 0 || g.N % 4 != 0) return COGS_E_INVALID;
    if (g.lda % 8 != 0 || g.ldw % 8 != 0 || g.lda < g.K || g.ldw < g.K) return COGS_E_INVALID;
    if (((uintptr_t)g.A | (uintptr_t)g.W) & 15) return COGS_E_INVALID;
    RowsArgs p;
    const int rc = cogs_fill_epi(g, &p.epi);
    if (rc != COGS_OK) return rc;
    p.A = (const bf16_t*)g.A; p.lda = g.lda;
    p.W = (const bf16_t*)g.W; p.ldw = g.ldw;
    p.M = g.M; p.N = g.N; p.K = g.K;
    // which form: a function of N alone (the reduction order of an output must not depend on M or on the data).
    // Fewer than 1024 column blocks (o / down / qkv: 224 .. 288): eight waves split k, so that a CU has eight waves'
    // loads in flight, not one's. From 4096 blocks on (lm_head) a wave takes two blocks per activation fragment.
    // The thresholds, KS = 8 and U = 4 / 2 are design-condition choices: no A/B of the forms has been run. Known costs
    // of the k-split form: 224 workgroups on 256 CUs for o / down, and at M = 16 a workgroup reads as many A bytes
    // from L2 (16 x K x 2) as weight bytes from HBM.
    const int nblk = (g.N + 15) / 16;
    if (nblk < 1024) hipLaunchKernelGGL((gemm_rows_kernel<8, 1, 4>), dim3(nblk), dim3(512), 0, st, p);
    else if (nblk < 4096) hipLaunchKernelGGL((gemm_rows_kernel<1, 1, 4>), dim3((nblk + 3) / 4), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_rows_kernel<1, 2, 2>), dim3((nblk + 7) / 8), dim3(256), 0, st, p);
    return COGS_LAUNCH_CHECK();
}
