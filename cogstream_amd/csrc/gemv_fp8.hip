// W8A16 weight-streaming GEMV for single-token decode:  y[1,N] = epilogue( scale[n] * (x[1,K] . Q[N,K]^T) ).
//
// The weights are OCP e4m3fn codes (one byte each) with ONE power-of-two scale per output row (cogstream_amd/weights.py,
// quantize_fp8_rows, is the specification); the activations stay bf16 / fp32 and the sums fp32. Everything around the
// dot product is csrc/gemv.hip's: a wave owns 4 (or 2) consecutive output rows, every weight byte is read exactly once
// with non-temporal loads straight into registers, x is re-read from L2, the Qwen2RMSNorm of x can run as a prologue
// (register-resident at K = 3584), the new K / V row goes straight into the cache, and the epilogue functions are the
// GEMM's (gemm_epilogue.h). What differs:
//   * a chunk is LW = 8 (or 16) weight BYTES per lane, i.e. 8 (16) elements: with 8-byte loads K = 3584 is 7 x 64 chunks,
//     the bf16 kernel's layout, and the x / gamma registers of the prologue line up with the weight chunks one to one;
//   * bf16: v_cvt_scalef32_pk_bf16_fp8 (scale operand 1.0) turns two codes into a packed bf16 pair -- every e4m3 value is a
//     bf16 value -- that feeds v_dot2c_f32_bf16 directly: 2 VALU per two products. fp32: v_cvt_pk_f32_fp8 + two fmas;
//   * the row scale multiplies the reduced fp32 sum once, in front of the epilogue. A power of two commutes with every
//     rounding of the sum, so the result is the one a kernel reading the dequantised weights q * 2^e would give with the
//     same summation order.
// The same file holds the device quantiser of the load path (row absmax -> scale -> nearest-even codes, and optionally the
// dequantised values written back for the M > 1 kernels), bit-equal to the host function.
#include "common.h"
#include "kernels.h"
#include "gemm_epilogue.h"
#include "debug.h"

namespace {

struct GemvFp8Args {
    const char* x;
    const uint8_t* W; long ldw;   // bytes = elements
    const float* scale;           // [N]
    int N, K;
    const void* rms_gamma;        // != null: x is RMS-normalised on the fly (Qwen2RMSNorm fused into the GEMV)
    float rms_eps;
    char* kv_k; char* kv_v; int kv_col0, kv_dim;   // != null: columns >= kv_col0 are the new K / V cache row
    EpiArgs epi;
};

typedef __attribute__((ext_vector_type(2))) __bf16 bf2_t;

// raw weight chunk of LW bytes
template <int LW> struct WRaw;
template <> struct WRaw<8> { typedef u32x2 type; };
template <> struct WRaw<16> { typedef u32x4 type; };

// Weights are read exactly once per token by exactly one CU: non-temporal, as in gemv.hip
template <int LW>
__device__ __forceinline__ typename WRaw<LW>::type ldw_nt(const uint8_t* q) {
    return __builtin_nontemporal_load(reinterpret_cast<const typename WRaw<LW>::type*>(q));
}

// the x operand of one chunk: LW elements, kept as dwords -- bf16: LW / 2 packed pairs, fp32: LW values
template <typename T, int LW> struct XChunk { static constexpr int ND = LW * (int)sizeof(T) / 4; uint32_t d[ND]; };

template <typename T, int LW>
__device__ __forceinline__ void ldx(const T* x, int chunk, XChunk<T, LW>& o) {
    constexpr int NL = XChunk<T, LW>::ND / 4;
    const u32x4* p = reinterpret_cast<const u32x4*>(x + (long)chunk * LW);
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const u32x4 v = p[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) o.d[4 * i + e] = v[e];
    }
}

template <typename T, int LW>
__device__ __forceinline__ float sumsq(const XChunk<T, LW>& c, float ss) {
#pragma unroll
    for (int i = 0; i < XChunk<T, LW>::ND; ++i) {
        if constexpr (sizeof(T) == 2) { const float a = bf_lo(c.d[i]), b = bf_hi(c.d[i]); ss += a * a; ss += b * b; }
        else { const float a = __uint_as_float(c.d[i]); ss += a * a; }
    }
    return ss;
}

// Qwen2RMSNorm on one chunk: weight * (x * rstd).to(T) rounded to T, the values of norm.hip and of gemv.hip's prologue
template <typename T, int LW>
__device__ __forceinline__ void rms_chunk(XChunk<T, LW>& x, const XChunk<T, LW>& g, float rstd) {
#pragma unroll
    for (int i = 0; i < XChunk<T, LW>::ND; ++i) {
        if constexpr (sizeof(T) == 2) {
            const uint32_t t = pack_bf2(bf_lo(x.d[i]) * rstd, bf_hi(x.d[i]) * rstd);
            x.d[i] = pack_bf2(bf_lo(g.d[i]) * bf_lo(t), bf_hi(g.d[i]) * bf_hi(t));
        } else {
            x.d[i] = __float_as_uint(__uint_as_float(g.d[i]) * (__uint_as_float(x.d[i]) * rstd));
        }
    }
}

// acc + sum over the chunk of code * x: one chain per output row, the order of additions of gemv.hip on 8-byte chunks
template <typename T, int LW>
__device__ __forceinline__ float dot_chunk(const typename WRaw<LW>::type& w, const XChunk<T, LW>& x, float acc) {
#pragma unroll
    for (int i = 0; i < LW / 4; ++i) {
        if constexpr (sizeof(T) == 2) {
            const bf2_t lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[i], 1.0f, false);
            const bf2_t hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[i], 1.0f, true);
            acc = __builtin_amdgcn_fdot2_f32_bf16(lo, __builtin_bit_cast(bf2_t, x.d[2 * i]), acc, false);
            acc = __builtin_amdgcn_fdot2_f32_bf16(hi, __builtin_bit_cast(bf2_t, x.d[2 * i + 1]), acc, false);
        } else {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
            const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
            acc = fmaf(lo[0], __uint_as_float(x.d[4 * i]), acc);
            acc = fmaf(lo[1], __uint_as_float(x.d[4 * i + 1]), acc);
            acc = fmaf(hi[0], __uint_as_float(x.d[4 * i + 2]), acc);
            acc = fmaf(hi[1], __uint_as_float(x.d[4 * i + 3]), acc);
        }
    }
    return acc;
}

// epilogue of 2 consecutive output columns n, n+1 (one rotary / SwiGLU pair): gemv.hip's, same arithmetic as epilogue4
template <typename T>
__device__ __forceinline__ void epilogue2_fp8(const EpiArgs& p, int n, float v0, float v1) {
    const T* bias = reinterpret_cast<const T*>(p.bias);
    if (bias) { v0 += ld_f<T>(bias + n); v1 += ld_f<T>(bias + n + 1); }
    if (p.rope_cos && n < p.rope_cols) {
        const int pi = (n % p.head_dim) >> 1;
        float c, sn;
        if (p.rope_sin) { c = p.rope_cos[pi]; sn = p.rope_sin[pi]; }
        else { c = p.rope_cos[2 * pi]; sn = p.rope_cos[2 * pi + 1]; }
        const float r0 = fmaf(-v1, sn, v0 * c);
        const float r1 = fmaf(v0, sn, v1 * c);
        v0 = r0; v1 = r1;
    }
    if (n < p.q_cols) { v0 *= p.q_scale; v1 *= p.q_scale; }
    if (p.act == COGS_ACT_GELU_TANH) { v0 = gelu_tanh_f(v0); v1 = gelu_tanh_f(v1); }
    else if (p.act == COGS_ACT_GELU_ERF) { v0 = gelu_erf_f(v0); v1 = gelu_erf_f(v1); }
    else if (p.act == COGS_ACT_SWIGLU) {
        st_f<T>(reinterpret_cast<T*>(p.C) + (n >> 1), silu_f(v0) * v1);
        return;
    }
    if (p.R) {
        const T* r = reinterpret_cast<const T*>(p.R);
        v0 += ld_f<T>(r + n); v1 += ld_f<T>(r + n + 1);
    }
    if (p.out_f32) { reinterpret_cast<float*>(p.C)[n] = v0; reinterpret_cast<float*>(p.C)[n + 1] = v1; }
    else { st_f<T>(reinterpret_cast<T*>(p.C) + n, v0); st_f<T>(reinterpret_cast<T*>(p.C) + n + 1, v1); }
}

// R output rows per wave, U chunks of LW bytes per row in flight per lane (R * U independent loads, kept raw until used; U only
// batches the loads: the order of additions, and so the result, is the same for every U)
template <typename T, int R, int U, int LW>
__global__ __launch_bounds__(256) void gemv_fp8_kernel(GemvFp8Args p) {
    typedef typename WRaw<LW>::type wraw_t;
    typedef XChunk<T, LW> xchunk_t;
    const int lane = threadIdx.x & 63;
    const int n = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (n >= p.N) return;
    const int nch = p.K / LW;
    const T* x = reinterpret_cast<const T*>(p.x);
    const T* gam = reinterpret_cast<const T*>(p.rms_gamma);
    const uint8_t* w[R];
    float sc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = min(n + r, p.N - 1);
        w[r] = p.W + (long)row * p.ldw;
        sc[r] = p.scale[row];
    }
    // the first batch of weight chunks is requested BEFORE the fused RMSNorm statistics (the weights do not depend on x)
    int ch = lane;
    wraw_t w_first[U][R];
    const bool have_first = ch + 64 * (U - 1) < nch;
    if (have_first) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r) w_first[u][r] = ldw_nt<LW>(w[r] + (long)(ch + 64 * u) * LW);
    }
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    auto finish = [&]() {
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]) * sc[r];
        if (lane == 0) {
            EpiArgs e = p.epi;
            if (p.kv_k && n >= p.kv_col0)   // region boundaries are multiples of 4: a wave's columns lie in one region
                e.C = (n < p.kv_col0 + p.kv_dim) ? p.kv_k - (long)p.kv_col0 * sizeof(T)
                                                 : p.kv_v - (long)(p.kv_col0 + p.kv_dim) * sizeof(T);
            if constexpr (R == 4) epilogue4<T>(e, 0, n, f32x4{acc[0], acc[1], acc[2], acc[3]});
            else epilogue2_fp8<T>(e, n, acc[0], acc[1]);
        }
    };
    float rstd = 1.f;
    // Fused Qwen2RMSNorm with K = 3584 (every fused call of the model: qkv, gate/up, lm_head) on 8-byte weight chunks: x and
    // gamma are 7 sixteen-byte chunks per lane, loaded ONCE right behind the first weight batch and used for the statistics and
    // for the products, as in gemv.hip
    constexpr int XC = 7;
    if constexpr (sizeof(T) == 2 && LW == 8 && U <= XC) {
        if (gam && nch == XC * 64) {
            xchunk_t xall[XC], gall[XC];
#pragma unroll
            for (int i = 0; i < XC; ++i) { ldx<T, LW>(x, lane + 64 * i, xall[i]); ldx<T, LW>(gam, lane + 64 * i, gall[i]); }
            float ss = 0.f;
#pragma unroll
            for (int i = 0; i < XC; ++i) ss = sumsq<T, LW>(xall[i], ss);
            ss = wave_sum(ss);
            rstd = rsqrtf(ss / (float)p.K + p.rms_eps);
#pragma unroll
            for (int i = 0; i < XC; ++i) rms_chunk<T, LW>(xall[i], gall[i], rstd);
#pragma unroll
            for (int b0 = 0; b0 < XC; b0 += U) {
                wraw_t wr[U][R];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (b0 + u < XC) wr[u][r] = b0 == 0 ? w_first[u][r] : ldw_nt<LW>(w[r] + (long)(lane + 64 * (b0 + u)) * LW);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (b0 + u >= XC) continue;
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r] = dot_chunk<T, LW>(wr[u][r], xall[b0 + u], acc[r]);
                }
            }
            finish();
            return;
        }
    }
    if (gam) {
        // every wave covers the whole x with its 64 lanes: the statistics need no LDS and no barrier
        float ss = 0.f;
        for (int c = lane; c < nch; c += 64) {
            xchunk_t xv;
            ldx<T, LW>(x, c, xv);
            ss = sumsq<T, LW>(xv, ss);
        }
        ss = wave_sum(ss);
        rstd = rsqrtf(ss / (float)p.K + p.rms_eps);
    }
    auto chunk = [&](int c, const wraw_t (&wr)[R]) {
        xchunk_t xv;
        ldx<T, LW>(x, c, xv);
        if (gam) {
            xchunk_t gv;
            ldx<T, LW>(gam, c, gv);
            rms_chunk<T, LW>(xv, gv, rstd);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = dot_chunk<T, LW>(wr[r], xv, acc[r]);
    };
    if (have_first) {
#pragma unroll
        for (int u = 0; u < U; ++u) chunk(ch + 64 * u, w_first[u]);
        ch += 64 * U;
    }
    for (; ch + 64 * (U - 1) < nch; ch += 64 * U) {
        wraw_t wr[U][R];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r) wr[u][r] = ldw_nt<LW>(w[r] + (long)(ch + 64 * u) * LW);
#pragma unroll
        for (int u = 0; u < U; ++u) chunk(ch + 64 * u, wr[u]);
    }
    for (; ch < nch; ch += 64) {
        wraw_t wr[R];
#pragma unroll
        for (int r = 0; r < R; ++r) wr[r] = ldw_nt<LW>(w[r] + (long)ch * LW);
        chunk(ch, wr);
    }
    finish();
}

// ---------------------------------------------------------------------------------------------- device quantiser

// value of an OCP e4m3fn code without its sign (NaN codes do not occur: the quantiser never writes them)
__device__ __forceinline__ float e4m3_magnitude(uint32_t c) {
    const int e = (c >> 3) & 15, m = c & 7;
    return e ? ldexpf((float)(8 + m), e - 10) : ldexpf((float)m, -9);
}

// nearest-even e4m3fn code of v, |v| <= 448 (larger magnitudes saturate to 448; the quantiser's scale keeps them out)
__device__ __forceinline__ uint32_t e4m3_rne(float v) {
    const uint32_t bits = __float_as_uint(v);
    const uint32_t sign = (bits >> 24) & 0x80u;
    const uint32_t mag = bits & 0x7fffffffu;
    uint32_t code;
    if (mag < 0x3c800000u) {                     // below 2^-6, the smallest normal: multiples of 2^-9 (8 = the smallest normal itself)
        code = (uint32_t)rintf(__uint_as_float(mag) * 512.0f);
    } else {
        const uint32_t r = (mag + 0x7ffffu + ((mag >> 20) & 1u)) >> 20;      // sign-less exponent | 3 mantissa bits, nearest even
        code = r - ((127u - 7u) << 3);
        if (code > 0x7eu) code = 0x7eu;
    }
    return sign | code;
}

// one wave per row: absmax -> scale = 2^ceil(log2(absmax / 448)) in integer arithmetic on the exponent -> codes (8 per lane and
// step); deq != null: the dequantised row in T as well (may be w itself: a lane rewrites only what it has read)
template <typename T>
__global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(const T* w, long ldw, int N, int K, uint8_t* codes, long ldq,
                                                                float* scale, T* deq, long ldd) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const T* wr = w + (long)row * ldw;
    const int nch = K / 8;
    float m = 0.f;
    for (int c = lane; c < nch; c += 64) {
        float v[8];
        ld8_f<T>(wr + c * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(v[e]));
    }
    m = wave_max(m);
    int ex = 0;
    if (m > 0.f) {
        int fx;
        const float fm = frexpf(m, &fx);            // m = fm * 2^fx, fm in [0.5, 1); 448 = 0.875 * 2^9
        ex = fm <= 0.875f ? fx - 9 : fx - 8;
        ex = ex < -126 ? -126 : ex;
    }
    const float s = ldexpf(1.0f, ex), inv = ldexpf(1.0f, -ex);
    if (lane == 0) scale[row] = s;
    uint8_t* qr = codes + (long)row * ldq;
    for (int c = lane; c < nch; c += 64) {
        float v[8];
        ld8_f<T>(wr + c * 8, v);
        uint32_t q[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = e4m3_rne(v[e] * inv);
        u32x2 o;
        o[0] = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
        o[1] = q[4] | q[5] << 8 | q[6] << 16 | q[7] << 24;
        *reinterpret_cast<u32x2*>(qr + c * 8) = o;
        if (deq) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = e4m3_magnitude(q[e] & 0x7f) * s;
                v[e] = (q[e] & 0x80) ? -d : d;
            }
            st8_f<T>(deq + (long)row * ldd + c * 8, v);
        }
    }
}

// deep: as many weight BYTES in flight per lane as the bf16 kernel (R * U * LW = 112 .. 128), else half of that
template <typename T, int LW>
int launch_fp8(hipStream_t st, const GemvFp8Args& p, bool small_n, bool deep) {
    constexpr int U2 = LW == 8 ? 4 : 2, U2D = LW == 8 ? 7 : 4;     // 2 rows per wave (7: all of K = 3584 at once)
    constexpr int U4 = LW == 8 ? 2 : 1, U4D = LW == 8 ? 4 : 2;     // 4 rows per wave
    if (small_n) {
        const dim3 grid((p.N / 2 + 3) / 4), blk(256);
        if (deep) hipLaunchKernelGGL((gemv_fp8_kernel<T, 2, U2D, LW>), grid, blk, 0, st, p);
        else hipLaunchKernelGGL((gemv_fp8_kernel<T, 2, U2, LW>), grid, blk, 0, st, p);
    } else {
        const dim3 grid((p.N / 4 + 3) / 4), blk(256);
        if (deep) hipLaunchKernelGGL((gemv_fp8_kernel<T, 4, U4D, LW>), grid, blk, 0, st, p);
        else hipLaunchKernelGGL((gemv_fp8_kernel<T, 4, U4, LW>), grid, blk, 0, st, p);
    }
    return COGS_LAUNCH_CHECK();
}

}  // namespace

// g: the descriptor of cogs_k_gemv with M = 1, W = the e4m3 codes and ldw in BYTES; g.dtype is the activations' type
int cogs_k_gemv_fp8(hipStream_t st, const CogsGemm& g, const float* scale) {
    if (g.dtype != COGS_DT_BF16 && g.dtype != COGS_DT_F32) return COGS_E_INVALID;
    if (!g.A || !g.W || !g.C || !scale) return COGS_E_INVALID;
    if (g.M != 1 || g.N <= 0 || g.K <= 0 || g.N % 4 || g.K % 16 || g.ldw % 16 || g.ldw < g.K) return COGS_E_INVALID;
    if (((uintptr_t)g.A | (uintptr_t)g.W | (uintptr_t)g.rms_gamma) & 15) return COGS_E_INVALID;
    if (g.row_stats || g.ln_ab || g.hm_rows > 0 || g.rope_lut) return COGS_E_UNSUPPORTED;
    GemvFp8Args p;
    const int rc = cogs_fill_epi(g, &p.epi);
    if (rc != COGS_OK) return rc;
    p.x = (const char*)g.A;
    p.W = (const uint8_t*)g.W; p.ldw = g.ldw;
    p.scale = scale;
    p.N = g.N; p.K = g.K;
    p.rms_gamma = g.rms_gamma; p.rms_eps = g.rms_eps;
    p.kv_k = (char*)g.kv_k; p.kv_v = (char*)g.kv_v; p.kv_col0 = g.kv_col0; p.kv_dim = g.kv_dim;
    if (g.kv_k && (!g.kv_v || g.kv_col0 % 4 || g.kv_dim % 4 || g.out_f32 || g.act == COGS_ACT_SWIGLU ||
                   g.kv_col0 + 2 * g.kv_dim != g.N)) return COGS_E_INVALID;
    // rows per wave as in gemv.hip (the same switch: the criterion is workgroups per CU, not bytes); load width and depth:
    // tools/decode_fp8_time.py --sweep
    const bool small_n = g.N / 16 < (int)g_cogs_debug.gemv_small_n;
    const bool wide = g_cogs_debug.gemv_fp8_load == 16, deep = g_cogs_debug.gemv_fp8_deep != 0;
    if (g.dtype == COGS_DT_BF16) return wide ? launch_fp8<bf16_t, 16>(st, p, small_n, deep) : launch_fp8<bf16_t, 8>(st, p, small_n, deep);
    return wide ? launch_fp8<float, 16>(st, p, small_n, deep) : launch_fp8<float, 8>(st, p, small_n, deep);
}

int cogs_k_quantize_fp8_rows(hipStream_t st, int dtype, const void* w, long ldw, int N, int K, uint8_t* codes, long ldq,
                             float* scale, void* deq, long ldd) {
    if (dtype != COGS_DT_BF16 && dtype != COGS_DT_F32) return COGS_E_INVALID;
    const int es = dtype == COGS_DT_BF16 ? 2 : 4;
    if (!w || !codes || !scale || N <= 0 || K <= 0 || K % 16 || ldw < K || ldq < K || ldq % 8 || (ldw * es) % 16) return COGS_E_INVALID;
    if (deq && (ldd < K || (ldd * es) % 16 || ((uintptr_t)deq & 15))) return COGS_E_INVALID;
    if (((uintptr_t)w & 15) || ((uintptr_t)codes & 7)) return COGS_E_INVALID;
    const dim3 grid((N + 3) / 4), blk(256);
    if (dtype == COGS_DT_BF16)
        hipLaunchKernelGGL((quantize_fp8_rows_kernel<bf16_t>), grid, blk, 0, st, (const bf16_t*)w, ldw, N, K, codes, ldq, scale, (bf16_t*)deq, ldd);
    else
        hipLaunchKernelGGL((quantize_fp8_rows_kernel<float>), grid, blk, 0, st, (const float*)w, ldw, N, K, codes, ldq, scale, (float*)deq, ldd);
    return COGS_LAUNCH_CHECK();
}
