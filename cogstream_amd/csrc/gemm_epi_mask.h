// Epilogue mask bits of the GEMM kernels and the list of masks that have a compile-time specialisation.
// Plain preprocessor text, no HIP: shared by the kernels (gemm_epilogue.h) and the host-only launch plan (gemm_plan.h).
#pragma once

#define EPI_BIAS 1
#define EPI_RES 2
#define EPI_ROPE 4
#define EPI_GELU_TANH 8
#define EPI_GELU_ERF 16
#define EPI_SWIGLU 32
#define EPI_F32OUT 64
#define EPI_GENERIC 128   // decide everything at run time (rare combinations)
#define EPI_ROPE_LUT 512  // with EPI_ROPE, ping-pong kernel only: rotary factors from the LDS-resident position LUT
#define EPI_NOSTORE 256   // diagnostics only (COGS_GEMM_NOSTORE): accumulators kept live, nothing written
// LayerNorm fused around the GEMMs (model/modeling_videollama3_encoder.py:382-391: x += attn(LN1(x)); x += mlp(LN2(x))):
//   EPI_ROWSTAT  the GEMM that PRODUCES the residual stream x (patch embed, out-proj, fc2; N = hidden) also writes, per
//                row and 64-column wave tile, the partial sums (sum x, sum x^2) of the values it STORES (the bf16-rounded
//                ones in bf16 mode: what the consumer will read): stat_part[M][N/64][2].
//                A tiny kernel turns them into (a, b) = (rstd, -rstd * mean) per row (cogs_k_ln_finalize).
//   EPI_LNFOLD   the GEMM that CONSUMES LN(x) reads x itself with W'' = rows of W * diag(gamma) CENTRED (their mean over k
//                subtracted, folded at load time: sum_k x_k W''[n][k] = sum_k (x_k - mean) W'[n][k]) and applies
//                y[r][n] = rstd_r * acc[r][n] + c_n, c_n = bias_n + sum_k beta_k W[n][k] -- algebraically LN(x) W^T + bias,
//                with no normalised copy of x ever written or read and no extra arithmetic in the epilogue (the bias add
//                becomes an fma). The term rstd * mean * (sum_k of the bf16-ROUNDED W'') is not evaluated: the packer
//                (weights.fold_layernorm) makes the rounded rows sum to zero as well, so there is nothing to neglect.
#define EPI_ROWSTAT 1024
#define EPI_LNFOLD 2048
// Head-major output (round 5; the ViT QKV GEMM): instead of C[m][n] the element of row m, column n goes to
//   C + ((n / hm_cols) * hm_rows * hm_cols  +  ((n % hm_cols) / hm_hd) * hm_rows * hm_hd  +  m * hm_hd  +  n % hm_hd)
// i.e. [q | k | v][head][row][head_dim]: every (head, frame) block of K and V is ONE contiguous run of rows, so the
// attention kernel's 1 KiB LDS-DMA pieces are whole 128-byte lines (54 B/clk per CU against 28 for the 144-byte runs at a
// 6 912-byte stride of the row-major layout: profiles/r4_ldsdma_rate.txt). 8 consecutive columns that start at a multiple
// of 8 never leave a head (hm_hd % 8 == 0), so the 16-byte stores of the wide paths stay whole.
#define EPI_HM 4096

// Every mask with its own instantiation of every kernel body; any other combination runs as EPI_GENERIC. The K-tile
// ping-pong body adds the EPI_ROPE_LUT forms of its rotary masks and EPI_NOSTORE (gemm.hip, dispatch_pp).
#define COGS_EPI_SPECIALISED(X)                                                                                              \
    X(0) X(EPI_BIAS) X(EPI_RES) X(EPI_BIAS | EPI_RES) X(EPI_BIAS | EPI_ROPE) X(EPI_BIAS | EPI_GELU_TANH)                   \
    X(EPI_BIAS | EPI_GELU_ERF) X(EPI_BIAS | EPI_ROWSTAT) X(EPI_BIAS | EPI_RES | EPI_ROWSTAT) X(EPI_BIAS | EPI_LNFOLD)      \
    X(EPI_BIAS | EPI_ROPE | EPI_LNFOLD) X(EPI_BIAS | EPI_GELU_TANH | EPI_LNFOLD) X(EPI_BIAS | EPI_ROPE | EPI_HM)           \
    X(EPI_BIAS | EPI_ROPE | EPI_LNFOLD | EPI_HM) X(EPI_SWIGLU) X(EPI_F32OUT)
