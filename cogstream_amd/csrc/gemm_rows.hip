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
//
// gemm_rows_fp8_kernel is the same kernel on OCP e4m3fn codes with one power-of-two fp32 scale per output column (what
// cogs_quantize_fp8_rows writes):  C[M,N] = epilogue( scale[n] * sum_k A[m,k] * e4m3(W[n,k]) ). Lane (r, g) loads the 16 code
// BYTES k = 64c + 16g .. + 15 of weight row r with one non-temporal load and turns them into the two bf16 fragments with
// v_cvt_scalef32_pk_bf16_fp8 (scale operand 1.0, as gemv_fp8.hip): bytes 0-7 are the fragment of MFMA h = 0, bytes 8-15 that of
// h = 1, so fragment element j of group g is k = 64c + 16g + 8h + j as above. Forms, thresholds, KS, the chunk -> wave map and
// the order of the LDS reduction are the bf16 kernel's (rows_pick_form is the only place that knows them), so every
// accumulator sees the same MFMAs on the same k sets in the same order as gemm_rows_kernel on the dequantised matrix
// code * scale, only with every weight 1 / scale[n] times as large. The scale multiplies the finished fp32 sum once (k-split:
// after wave 0's ordered add), in front of epilogue4(). Every e4m3 value is a bf16 value and a power of two commutes with
// every rounding, so the result is BIT-IDENTICAL to cogs_k_gemm_rows on the dequantised matrix -- that is the contract
// (one model whichever weights a step streams) -- wherever the dequantised weights code * scale are normal bf16
// numbers and the sums (partial sums included) times scale are normal fp32 numbers: a subnormal on either side is rounded
// (or flushed) on one side only.
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

// ---- the same kernel on e4m3 codes (see the head of the file)
struct RowsFp8Args {
    const bf16_t* A; long lda;     // elements
    const uint8_t* W; long ldw;    // bytes = elements
    const float* scale;            // [N]
    int M, N, K;
    EpiArgs epi;
};

typedef __attribute__((ext_vector_type(2))) __bf16 bf2_t;

// eight codes (two dwords, k ascending with the byte address) -> the bf16 fragment of one MFMA
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(uint32_t lo, uint32_t hi) {
    u32x4 f;
    f[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));   // bytes 0, 1
    f[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));    // bytes 2, 3
    f[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
    f[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
    return __builtin_bit_cast(bf16x8, f);
}

// KS, CB: as gemm_rows_kernel (they fix the order of additions); U only batches the loads
template <int KS, int CB, int U>
__global__ __launch_bounds__(KS == 1 ? 256 : 64 * KS) void gemm_rows_fp8_kernel(RowsFp8Args p) {
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
    const uint8_t* wp[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) wp[cb] = p.W + (long)min(n0 + 16 * cb + r, p.N - 1) * p.ldw + 16 * g;
    const bool a_on = r < p.M;
    const bf16_t* ap = p.A + (long)min(r, p.M - 1) * p.lda + 16 * g;

    // the scales of the lane's four output columns, requested in front of the weight stream by the waves that store
    f32x4 sc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) sc[cb] = f32x4{1.f, 1.f, 1.f, 1.f};
    if (KS == 1 || wid == 0) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) sc[cb][i] = p.scale[min(n0 + 16 * cb + 4 * g + i, p.N - 1)];
    }

    struct Batch { u32x4 w[U][CB]; u32x4 a[U][2]; };
    auto load = [&](Batch& b, int c0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * KS;              // wave-uniform
            if (c < nch) {
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
                    b.w[u][cb] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[cb] + c * 64));
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    b.a[u][h] = u32x4{0, 0, 0, 0};
                    if (a_on) b.a[u][h] = *reinterpret_cast<const u32x4*>(ap + c * 64 + 8 * h);
                }
            } else {
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) b.w[u][cb] = u32x4{0, 0, 0, 0};
#pragma unroll
                for (int h = 0; h < 2; ++h) b.a[u][h] = u32x4{0, 0, 0, 0};
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
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(e4m3x8_to_bf16(cur.w[u][cb][2 * h], cur.w[u][cb][2 * h + 1]),
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
        if (n < p.N) epilogue4<bf16_t>(p.epi, r, n, acc[cb] * sc[cb]);
    }
}

// which form: a function of N alone (the reduction order of an output must not depend on M or on the data), and the ONE
// place that chooses it, for the bf16 and the e4m3 kernel alike: launch(RowsForm<KS, CB>, grid, block).
// Fewer than 1024 column blocks (o / down / qkv: 224 .. 288): eight waves split k, so that a CU has eight waves'
// loads in flight, not one's. From 4096 blocks on (lm_head) a wave takes two blocks per activation fragment.
// The thresholds and KS = 8 are design-condition choices: no A/B of the forms has been run. Known costs
// of the k-split form: 224 workgroups on 256 CUs for o / down, and at M = 16 a workgroup reads as many A bytes
// from L2 (16 x K x 2) as weight bytes from HBM.
template <int KS_, int CB_> struct RowsForm { static constexpr int KS = KS_, CB = CB_; };
template <class Launch>
void rows_pick_form(int N, Launch launch) {
    const int nblk = (N + 15) / 16;
    if (nblk < 1024) launch(RowsForm<8, 1>{}, dim3(nblk), dim3(512));
    else if (nblk < 4096) launch(RowsForm<1, 1>{}, dim3((nblk + 3) / 4), dim3(256));
    else launch(RowsForm<1, 2>{}, dim3((nblk + 7) / 8), dim3(256));
}

// what both launchers refuse: first what no multi-row kernel exists for, then the shapes (ld_mult: elements of W per 16 bytes)
int rows_check(const CogsGemm& g, int ld_mult) {
    if (g.dtype != COGS_DT_BF16 || g.M > 16) return COGS_E_UNSUPPORTED;
    if (g.ln_ab || g.row_stats || g.hm_rows > 0 || g.rope_lut || g.rms_gamma || g.kv_k ||
        g.act == COGS_ACT_GELU_TANH || g.act == COGS_ACT_GELU_ERF)
        return COGS_E_UNSUPPORTED;
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.K % 64 != 0 || g.N % 4 != 0) return COGS_E_INVALID;
    if (g.lda % 8 != 0 || g.ldw % ld_mult != 0 || g.lda < g.K || g.ldw < g.K) return COGS_E_INVALID;
    if (((uintptr_t)g.A | (uintptr_t)g.W) & 15) return COGS_E_INVALID;
    return COGS_OK;
}

}  // namespace

int cogs_k_gemm_rows(hipStream_t st, const CogsGemm& g) {
    int rc = rows_check(g, 8);
    if (rc != COGS_OK) return rc;
    RowsArgs p;
    rc = cogs_fill_epi(g, &p.epi);
    if (rc != COGS_OK) return rc;
    p.A = (const bf16_t*)g.A; p.lda = g.lda;
    p.W = (const bf16_t*)g.W; p.ldw = g.ldw;
    p.M = g.M; p.N = g.N; p.K = g.K;
    // U = 4 / 2 chunks per batch: a design-condition choice like the forms
    rows_pick_form(g.N, [&](auto f, dim3 grid, dim3 blk) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((gemm_rows_kernel<F::KS, F::CB, F::CB == 1 ? 4 : 2>), grid, blk, 0, st, p);
    });
    return COGS_LAUNCH_CHECK();
}

// g: the descriptor of cogs_k_gemm_rows with W = the e4m3 codes and ldw in BYTES
int cogs_k_gemm_rows_fp8(hipStream_t st, const CogsGemm& g, const float* scale) {
    int rc = rows_check(g, 16);
    if (rc != COGS_OK) return rc;
    if (!scale) return COGS_E_INVALID;
    RowsFp8Args p;
    rc = cogs_fill_epi(g, &p.epi);
    if (rc != COGS_OK) return rc;
    p.A = (const bf16_t*)g.A; p.lda = g.lda;
    p.W = (const uint8_t*)g.W; p.ldw = g.ldw;
    p.scale = scale;
    p.M = g.M; p.N = g.N; p.K = g.K;
    // U = 2 in every form: 2 (one block per wave) or 4 (two blocks) weight loads of 16 bytes per lane and batch where the bf16
    // kernel has 8, in 72-104 registers instead of 132-148. Swept as U = 4 / 4 / 2, 2 / 2 / 1 and 8 / 8 / 4 for the
    // three forms (profiles/decode_rows_fp8_time.txt): the two one-block forms are fastest at 2, the two-block form (lm_head) at 2
    // as well (1: +20 %), 8 / 8 / 4 is slower everywhere. U only batches the loads: the bits do not depend on it
    rows_pick_form(g.N, [&](auto f, dim3 grid, dim3 blk) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((gemm_rows_fp8_kernel<F::KS, F::CB, 2>), grid, blk, 0, st, p);
    });
    return COGS_LAUNCH_CHECK();
}
