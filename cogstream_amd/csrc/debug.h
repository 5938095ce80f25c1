// Diagnostic switches of libcogs_hip.so: ONE table, changed only through cogs_debug_set (include/cogs.h).
//
// Nothing in the library reads the environment. Every entry below has the SHIPPED behaviour as its default; the
// measurement tools (bench.py --debug, tools/*) and the A/B tests flip an entry by name, run, and flip it back -- in one
// process, so both sides of a comparison run on the same device (rounds 1-4 read ~28 COGS_* environment variables into
// function-local statics spread over the kernel files; a value could only be chosen before the first call).
// The table is process-wide. Its entries are relaxed atomics: another host thread driving its own handle may read a switch (or
// write one of the two last_* reports) while this one sets it without a data race -- which value a call running at that moment
// sees is still unspecified, so set a switch between calls. cogs_debug_set checks the value against the entry's range
// (csrc/capi.hip) and warns on stderr when a timing-only switch that changes results is turned on.
#pragma once
#include <atomic>

//   X(name, default, meaning)
#define COGS_DEBUG_SWITCHES(X)                                                                                              \
    /* ---- GEMM (csrc/gemm.hip) ---- */                                                                                    \
    X(gemm_pp64, 1, "1: whole-line ping-pong kernel (gemm_tn_pp64_kernel); 0: the 32-wide K-tile body it replaced")         \
    X(gemm_tall, 1, "whole-line kernel: 1 a ragged column block of <= 128 columns as 384x128 tiles (round 6), 0 as padded 256x256 tiles") \
    X(gemm_even_grid, 0, "whole-line kernel: 1 the fewest persistent workgroups that keep the round count (every workgroup the same number of tiles), 0 always 256") \
    X(gemm_pingpong, 1, "0: never take a ping-pong kernel (256x128 ring / 128x128 kernels only)")                          \
    X(gemm_small, 0, "1: always the 128x128 kernel")                                                                        \
    X(gemm_wgs, 256, "persistent workgroups of the 256x128 ring kernel (0: one tile per workgroup)")                        \
    X(gemm_pad_pct, 112, "ping-pong kernel is taken while N padded to 256 <= this percentage of N")                         \
    X(gemm_rope_lut, 1, "K-tile body only: rotary factors from the LDS position LUT when the caller supplies one")          \
    X(gemm_group_m, 0, "> 0: row blocks per group of the ping-pong tile walk (0: chosen per shape)")                        \
    X(gemm_split, 1, "0: no round-aligned / few-tile split of a launch")                                                    \
    X(gemm_co_streams, 0, "> 0: overrides the co-running-streams hint of the few-tile choice")                              \
    X(gemm_ring_cost_permille, 720, "few-tile choice: cost of a round of ring tiles relative to a round of ping-pong tiles") \
    X(gemm_epi_serial, 0, "1: the two wave groups' epilogues in separate intervals (the order before round 4)")             \
    X(gemm_nostore, 0, "1: timing only -- K loops without epilogues (results are NOT written)")                             \
    X(gemm_trace, 0, "1: per-tile s_memtime stamps of workgroup 0 printed to stderr (K-tile body only; synchronises)")      \
    X(gemm_choice, 0, "1: print which body every ping-pong-eligible shape gets")                                            \
    X(gemm_headmajor, 1, "ViT encode: QKV GEMM writes q/k/v head-major [which][head][row][hd] for the attention kernel")    \
    X(gemv_small_n, 1024, "GEMV: 2 output rows per wave while N / 16 is below this (else 4)") \
    X(gemv_dot2, 1, "bf16 GEMV (decode): 1 products on v_dot2c_f32_bf16 from the packed registers (round 5), 0 unpack + fp32 fma per element") \
    X(gemv_fp8_load, 8, "e4m3 GEMV (csrc/gemv_fp8.hip): bytes per weight load, 8 (K = 3584 is 7 x 64 chunks: register-resident fused RMSNorm) or 16") \
    X(gemv_fp8_deep, 0, "e4m3 GEMV: 1 as many weight bytes in flight per lane as the bf16 GEMV (twice the loads), 0 as many loads (half the bytes; measured faster)") \
    /* ---- attention (csrc/attn.hip, attn_vit.hip, attn_decode.hip) ---- */                                                \
    X(attn_vit, 2, "ViT block-diagonal attention: 2 pipelined LDS-DMA kernel, 1 unpipelined, 0 general kernel")            \
    X(attn_vit_early, 0, "1: pipelined ViT kernel issues tiles 1-2 before its first wait (the order before round 4)")       \
    X(attn_vit_len, 1, "ViT attention: 0 the run-time form of the ragged end also for one-video launches (round 6: its shape as template parameters)") \
    X(attn_uniform_hint, 0, "tests: > 0 = cogs_attention treats every cu_seqlens segment as exactly this many rows (the hint cogs_vit_encode derives from the grid itself)") \
    X(attn_decode, 1, "0: single-token attention through the general split-KV kernel")                                      \
    X(attn_combine32, 1, "split-KV combine: 1 one block per (head, 32-column slice), 8 loads in flight per thread; 0 one block per head") \
    X(attn_prefill_dma, 1, "0: Qwen2 prompt attention through the general register-staged kernel")                          \
    X(attn_light_first, 0, "1: causal query tiles issued lightest first")                                                   \
    X(attn_nq, 0, "general kernel: 1 / 2 forces 16 / 32 query rows per wave")                                              \
    /* ---- encoder / LLM drivers (csrc/capi_vit.hip, capi_llm.hip), k-means */                                            \
    X(vit_split_max, 1099511627776LL, "clips above this many patches are encoded on one stream")                           \
    X(llm_split_keys, 0, "> 0: keys per split of the decode attention (0: chosen from the context)")                        \
    X(llm_decode_fp8, 1, "cogs_llm_forward with e4m3 weights attached (cogs_llm_attach_fp8): 1 single-token steps read them, 0 the dequantised bf16 / fp32 copy (the in-process A/B)") \
    X(llm_rows_fp8, 1, "cogs_llm_decode_rows / _slots with e4m3 weights attached: 1 the multi-row step streams the codes (cogs_gemm_rows_fp8; measured faster at every R), 0 the dequantised bf16 copy (the in-process A/B; the same bits either way)") \
    X(beam_gather_tails, 0, "tests: 1 = beam search (llm.py, read through cogs_debug_get) copies every beam's tail behind its parent's per step and passes no slot table; 0 the tails stay where they were written and cogs_attention_rows reads them through the table") \
    X(km_row_groups, 0, "> 0: row groups of the k-means distance pass (0: sized to fill the chip)")                       \
    /* ---- teacher-forced scoring (csrc/lm_score.hip) ---- */                                                              \
    X(lm_score_rows, 2048, "cogs_lm_score / cogs_row_lse: rows of a logits panel")                                          \
    X(lm_score_cols, 0, "> 0: columns of a logits panel, rounded down to 32 (0: what a 64 MiB panel holds; never more than that)") \
    X(lm_score_split, 0, "> 0: workgroups per panel row of the fold kernel (0: about 1024 workgroups while a panel has < 512 rows, else 1)")

struct CogsDebug {
#define COGS_DBG_FIELD(name, dflt, doc) std::atomic<long long> name{dflt};
    COGS_DEBUG_SWITCHES(COGS_DBG_FIELD)
#undef COGS_DBG_FIELD
    // read-only reports (cogs_debug_get): what the last cogs_gemm of this process dispatched to
    // 0 none yet, 1 128x128, 2 256x128 ring, 3 K-tile ping-pong, 4 whole-line ping-pong, 5 ping-pong + ring (split), 6 GEMV
    std::atomic<long long> gemm_last_body{0};
    // ... and the last cogs_attention: 1 general MFMA kernel, 2 ViT unpipelined, 3 ViT pipelined (row-major K/V), 4 single-token
    // decode (+ combine), 5 prompt LDS-DMA kernel, 7 row-wise fp32 kernel, 8 ViT pipelined, head-major K/V (6 and 9 were the archived
    // ping-pong / 64-rows-per-wave prompt kernels: tools/experiments/attn_prefill_variants.hip)
    std::atomic<long long> attn_last_kernel{0};
    // ... and which ragged end the last pipelined ViT launch had: 10 R + blocks of the last tile (41 .. 72), 0 = the run-time form
    std::atomic<long long> attn_vit_last_end{0};
    // ... and how the last cogs_lm_score / cogs_row_lse walked its logits: workgroups per row of a full panel (1 = no column
    // split) and the columns each of them folds, and the panel shape
    std::atomic<long long> lm_score_last_split{0};
    std::atomic<long long> lm_score_last_chunk{0};
    std::atomic<long long> lm_score_last_rows{0};
    std::atomic<long long> lm_score_last_cols{0};
    // ... and whether the last cogs_llm_forward / _segments took the e4m3 GEMVs (1) or the weights' own dtype (0)
    std::atomic<long long> llm_last_decode_fp8{0};
    // ... and whether the last cogs_llm_decode_rows / _slots streamed the e4m3 codes (1) or the (dequantised) bf16 matrices (0)
    std::atomic<long long> llm_last_rows_fp8{0};
    // ... and which path the last cogs_sample took: 0 none yet, 1 slice top-k + merge (0 < top_k <= 64), 2 whole-row
    std::atomic<long long> sample_last_path{0};
};
extern CogsDebug g_cogs_debug;     // capi.hip
