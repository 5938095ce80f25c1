// Launch plan of cogs_k_gemm: which kernel body a shape gets, how its tiles are walked, the persistent grid, and whether
// the launch is split into whole rounds of ping-pong tiles plus a ring-kernel remainder. Host integer arithmetic only: no
// HIP, compiles with the host C++ compiler (tests/test_gemm_plan.py pins it on the CPU against tests/golden/gemm_plan.json).
#pragma once
#include <math.h>
#include "gemm_epi_mask.h"

// ---- tile geometry (the kernels in gemm.hip are built on the same constants) ----
constexpr int BM = 128;                 // 128x128 kernel
constexpr int BN = 128;                 //   ... and the columns of a 256x128 ring tile
constexpr int BM2 = 256;                // rows of a 256x128 ring tile
constexpr int BM3 = 256, BN3 = 256;     // ping-pong tile
constexpr int TALL4 = 384;              // rows of a tall tile (its columns: the <= 128 of the ragged column block)
constexpr int PERSISTENT_WGS = 256;     // one workgroup per CU (MI355X: 256 CUs)
constexpr int GROUP_M = 8;              // row blocks per group of the tile walk

// the gemm_* switches of debug.h that the plan reads, at their shipped defaults
struct GemmTuning {
    long long gemm_pp64 = 1, gemm_tall = 1, gemm_even_grid = 0, gemm_pingpong = 1, gemm_small = 0, gemm_wgs = 256,
              gemm_pad_pct = 112, gemm_rope_lut = 1, gemm_group_m = 0, gemm_split = 1, gemm_co_streams = 0,
              gemm_ring_cost_permille = 720, gemm_nostore = 0;
};

struct GemmQuery {
    bool bf16 = true;            // dtype: COGS_DT_BF16 (else fp32)
    int M = 0, N = 0, K = 0;
    int epi_mask = 0;            // cogs_epi_mask of the descriptor
    bool force_small_tile = false;
    bool rope_lut = false;       // the caller supplied a rotary LUT with row positions and an interleaved (cos, sin) table ...
    int rope_lut_bytes = 0;      //   ... of this size (0: too many positions for the 16-bit row fields)
    int co_streams = 1;          // streams the caller feeds with GEMMs of this size at the same time
};

// one kernel launch. body: the gemm_last_body numbering (1 128x128, 2 256x128 ring, 3 K-tile ping-pong, 4 whole-line
// ping-pong, 6 GEMV); 0 = no launch
struct GemmLaunch {
    int body = 0;
    int rows = 0;                // rows of the GEMM this launch computes
    int nbm = 0, nbn = 0;        // row / column blocks (tall: nbn counts the WHOLE column blocks only)
    int ntiles = 0;
    int group_m = GROUP_M;       // ping-pong bodies: row blocks per group of the tile walk
    int cf = 0;                  // whole-line body: tiles of a full group
    bool tall = false;           // whole-line body: the ragged column block as 384x128 tiles
    int grid = 0;                // workgroups
    bool rope_lut = false;       // the epilogue mask gains EPI_ROPE_LUT
    bool nostore = false;        // the epilogue mask becomes EPI_NOSTORE (timing only)
};

struct GemmPlan {
    GemmLaunch main, rest;       // rest.body != 0: rows [rows_main, M) go to a second launch (ring kernel)
    int rows_main = 0;
    int body = 0;                // what gemm_last_body reports: main.body, or 5 for a split
    // the ping-pong candidate behind the choice (`gemm_choice` print-out): its tiles = pp_rounds * 256 + pp_rem; mb_main
    // -1 unsplit ping-pong launch, 0 the whole GEMM to the ring kernel, > 0 row blocks that stay in the ping-pong kernel
    bool pp_eligible = false;
    int pp_tiles = 0, pp_rounds = 0, pp_rem = 0, mb_main = -1;
};

// Persistent workgroups of the whole-line kernel for `tiles` tiles. 256 = one per CU; switch gemm_even_grid = 1: the
// fewest workgroups (a multiple of 8: the tile walk is XCD-aware) that still finish in ceil(tiles / 256) rounds, so that every
// workgroup walks the same number of tiles and the CUs the last round would leave idle are free from the start -- for the
// other stream's kernel, or for the clock.
inline int cogs_pp64_grid(int tiles, const GemmTuning& t) {
    if (tiles <= PERSISTENT_WGS) return tiles;
    if (t.gemm_even_grid == 0) return PERSISTENT_WGS;
    const int rounds = (tiles + PERSISTENT_WGS - 1) / PERSISTENT_WGS;
    const int wgs = ((tiles + rounds - 1) / rounds + 7) / 8 * 8;
    return wgs < PERSISTENT_WGS ? wgs : PERSISTENT_WGS;
}

// the 128x128 kernel (one tile per workgroup) or the persistent 256x128 ring kernel on `rows` rows
inline GemmLaunch cogs_plan_ring(int rows, int N, bool big, const GemmTuning& t) {
    GemmLaunch l;
    l.body = big ? 2 : 1;
    l.rows = rows;
    l.nbm = (rows + (big ? BM2 : BM) - 1) / (big ? BM2 : BM);
    l.nbn = (N + BN - 1) / BN;
    l.ntiles = l.grid = l.nbm * l.nbn;
    const int wgs = (int)t.gemm_wgs;       // 0 = one tile per workgroup
    if (big && wgs > 0 && wgs < l.grid) l.grid = wgs;
    return l;
}

inline GemmPlan cogs_plan_gemm(const GemmQuery& q, const GemmTuning& t) {
    GemmPlan plan;
    if (q.M == 1) {
        plan.main.body = plan.body = 6; plan.main.rows = plan.rows_main = 1;
        return plan;
    }
    const bool small = t.gemm_small != 0;
    // debug switch gemm_pp64 = 0 keeps the 32-wide K-tile kernel (A/B runs); default: the whole-line kernel wherever it exists
    // (every epilogue but the rotary LUT one, for which it has no LDS left -- the rotary factors then come from global
    // memory instead: measured 1 % faster end to end than the LUT epilogue on the old body)
    const bool pp64 = t.gemm_pp64 != 0;
    const int n_pad = (q.N + BN3 - 1) / BN3 * BN3;
    const bool pp_fits = n_pad * 100 <= q.N * (int)t.gemm_pad_pct;   // default: <= 12 % of the MFMAs spent on N padding (N = 1152 -> 1280 measured faster than the 256x128 ring kernel)
    if (t.gemm_pingpong == 0 || small || !q.bf16 || q.M < 1024 || !pp_fits || q.force_small_tile) {
        plan.main = cogs_plan_ring(q.M, q.N, q.M >= 512 && !q.force_small_tile && !small, t);
        plan.rows_main = q.M; plan.body = plan.main.body;
        return plan;
    }
    GemmLaunch pp;
    pp.rows = q.M;
    pp.nbm = (q.M + BM3 - 1) / BM3;
    pp.nbn = (q.N + BN3 - 1) / BN3;
    const bool nostore = t.gemm_nostore != 0;
    // Tall tiles for a ragged column block of <= 128 columns (whole-line kernel only; see TALL4): nbn then counts the
    // whole column blocks, and a group of the walk must be a whole number of 384-row tiles.
    const int ragged_cols = q.N % BN3;
    const bool tall = t.gemm_tall != 0 && pp64 && q.K >= 128 && q.N > BN3 && ragged_cols > 0 && ragged_cols <= 128;
    pp.tall = tall;
    if (tall) pp.nbn = q.N / BN3;
    // tile walk: groups of group_m row blocks x all column blocks. Measured (in-run A/B, cfg2 shapes): few column
    // blocks with a long K (fc2: 5 x K 4352) want small groups (2: 0.627 -> 0.591 ms), many column blocks with a
    // short K (fc1: 17 x K 1152) want 8 (2: +7 %)
    const int gm = (int)t.gemm_group_m;
    const bool few_cols_long_k = (q.N + BN3 - 1) / BN3 <= 6 && q.K >= 2048;
    pp.group_m = gm > 0 ? gm : (few_cols_long_k ? 2 : GROUP_M);
    if (tall) pp.group_m = gm > 0 ? (gm + 2) / 3 * 3 : (few_cols_long_k ? 3 : 6);
    pp.cf = pp.group_m * pp.nbn + (tall ? pp.group_m * BM3 / TALL4 : 0);
    // tiles of the first `rows` rows (a whole number of row blocks, or all of M)
    auto count_tiles = [&](int rows) {
        const int nbm = (rows + BM3 - 1) / BM3;
        const int full = nbm / pp.group_m, last = nbm % pp.group_m;
        int n = full * pp.cf + last * pp.nbn;
        if (tall && last) n += (rows - full * pp.group_m * BM3 + TALL4 - 1) / TALL4;
        return n;
    };
    // row blocks (with tall tiles: a multiple of three = whole tall tiles) whose tiles number at most `tiles`
    auto whole_blocks = [&](int tiles) {
        return tall ? tiles * 3 / (3 * pp.nbn + 2) / 3 * 3 : tiles / pp.nbn;
    };
    if ((q.epi_mask & ~EPI_LNFOLD) == (EPI_BIAS | EPI_ROPE) && q.rope_lut && t.gemm_rope_lut != 0 && !pp64)
        pp.rope_lut = q.rope_lut_bytes > 0 && q.rope_lut_bytes <= 28 * 1024;
    // Round-aligned split. The persistent kernel walks its tiles with 256 workgroups; when the last round
    // is mostly empty (N = 1152 at cfg2: 1155 tiles = 4.5 rounds, half the CUs idle for a whole tile time) the
    // leading row blocks that make up WHOLE rounds stay here and the remaining rows go to the 256x128 kernel,
    // whose half-size tiles fill the chip again (rows are independent: same arithmetic per row, same K order, so
    // a row's result does not depend on which kernel computed it).
    const bool nosplit = t.gemm_split == 0;
    const int nb = count_tiles(q.M);
    const int rounds = nb / PERSISTENT_WGS, rem = nb % PERSISTENT_WGS;
    int mb_main = -1;      // >= 0: row blocks that stay in the ping-pong kernel (0 = none: the whole GEMM goes to the ring kernel)
    // (calibrated on K = 1152 .. 4352, the ViT shapes; longer K -- the Qwen2 prompt pass at M = 2048 -- keeps the
    // plain ping-pong launch)
    const int S = t.gemm_co_streams > 0 ? (int)t.gemm_co_streams : (q.co_streams < 1 ? 1 : q.co_streams);   // the switch: A/B runs
    if (!nosplit && !nostore && nb <= 2 * PERSISTENT_WGS && q.K <= 4352) {
        // Few tiles (one rank's share of a frame-sharded clip: M = 6 400 is 125 tiles for N = 1152 and 350 = 1.37
        // rounds for QKV): the time is rounds x one tile, so the choice is by rounds. Calibrated on the four ViT
        // shapes at M = 3 200 .. 14 784 (tools/cal_tiles.sh, rocprofv3; round 4 with the whole-line kernel,
        // tools/experiments/cring_sweep.sh): a round of 256x128 ring tiles takes 0.72 of a round of ping-pong tiles of
        // the same K; a second launch costs about 0.08 of one. With a second stream running the other half of the clip
        // (S = 2) the CUs a launch leaves idle are not lost, so a launch costs max(1, its share of the chip) and is never
        // split: measured at 3 200 / 3 696 / 6 400 / 14 784 rows per stream, the ring kernel wins the first two (65 and
        // 75 ping-pong tiles: -2 %, -7 % of the step), the ping-pong kernel the third (125 tiles: -12 %) and the unsplit
        // launch the last (-4 %).
        const int rbm = (q.M + BM2 - 1) / BM2, rbn = (q.N + BN - 1) / BN;
        auto launch_cost = [&](int tiles) {
            return S == 1 ? (float)((tiles + PERSISTENT_WGS - 1) / PERSISTENT_WGS)
                          : fmaxf(1.f, (float)S * (float)tiles / (float)PERSISTENT_WGS);
        };
        const float c_ring = (float)t.gemm_ring_cost_permille * 1e-3f;   // 0.72; the switch is for calibration sweeps
        const float c_launch = 0.08f;
        const float cost_pp = launch_cost(nb);
        const float cost_ring = c_ring * launch_cost(rbm * rbn);
        float best = cost_pp;
        if (cost_ring < best) { best = cost_ring; mb_main = 0; }
        if (S == 1 && rounds == 1 && rem > 0) {
            const int mb = whole_blocks(PERSISTENT_WGS);           // whole row blocks inside the first round
            const int rows_rem = q.M - mb * BM3;
            if (mb > 0 && rows_rem >= 512) {     // the remainder must reach the 256x128 ring kernel the cost model prices
                const float cost_split = 1.f + c_ring * launch_cost(((rows_rem + BM2 - 1) / BM2) * rbn) + c_launch;
                if (cost_split < best) { best = cost_split; mb_main = mb; }
            }
        }
    } else if (S == 1 && !nosplit && !nostore && q.K >= 2048 && rounds >= 2 && rem > 0 && rem * 100 < PERSISTENT_WGS * 45) {
        // (many tiles: pays when a tile is long against a second launch and the last round is less than ~45 % full:
        // measured with the two-segment K loop at K = 1152: -2 %; K = 3584, last round 34 % full: +2 %; K = 18944,
        // 34 %: +6 %; K = 4352, 51 % full (ViT fc2): -2 %, so it no longer splits)
        const int mb = whole_blocks(rounds * PERSISTENT_WGS);    // whole row blocks within the full rounds
        if (mb > 0 && q.M - mb * BM3 >= 512) mb_main = mb;
    }
    plan.pp_eligible = true;
    plan.pp_tiles = nb; plan.pp_rounds = rounds; plan.pp_rem = rem; plan.mb_main = mb_main;
    if (mb_main == 0) {       // M >= 1024 rows: the ring kernel
        plan.main = cogs_plan_ring(q.M, q.N, true, t);
        plan.rows_main = q.M; plan.body = plan.main.body;
        return plan;
    }
    if (mb_main > 0) {
        pp.rows = mb_main * BM3; pp.nbm = mb_main;
        plan.rest = cogs_plan_ring(q.M - pp.rows, q.N, true, t);      // >= 512 rows
    }
    pp.ntiles = count_tiles(pp.rows);
    pp.body = pp64 && q.K >= 128 && !pp.rope_lut ? 4 : 3;
    pp.grid = pp.body == 4 ? cogs_pp64_grid(pp.ntiles, t) : (pp.ntiles < PERSISTENT_WGS ? pp.ntiles : PERSISTENT_WGS);
    pp.nostore = nostore;
    plan.main = pp;
    plan.rows_main = pp.rows;
    plan.body = mb_main > 0 ? 5 : pp.body;
    return plan;
}
