// C entry points over csrc/gemm_plan.h for tests/test_gemm_plan.py (built with the host C++ compiler, loaded with ctypes)
#include "gemm_plan.h"

namespace {
long long* fields(GemmTuning& t, int i) {
    long long* f[] = {&t.gemm_pp64, &t.gemm_tall, &t.gemm_even_grid, &t.gemm_pingpong, &t.gemm_small, &t.gemm_wgs, &t.gemm_pad_pct,
                      &t.gemm_rope_lut, &t.gemm_group_m, &t.gemm_split, &t.gemm_co_streams, &t.gemm_ring_cost_permille, &t.gemm_nostore};
    return f[i];
}
void put(const GemmLaunch& l, int* o) {
    const int v[] = {l.body, l.rows, l.nbm, l.nbn, l.ntiles, l.group_m, l.cf, l.tall, l.grid, l.rope_lut};
    for (int i = 0; i < 10; ++i) o[i] = v[i];
}
}  // namespace

extern "C" const char* plan_tuning_names() {
    return "gemm_pp64 gemm_tall gemm_even_grid gemm_pingpong gemm_small gemm_wgs gemm_pad_pct gemm_rope_lut gemm_group_m gemm_split "
           "gemm_co_streams gemm_ring_cost_permille gemm_nostore";
}
extern "C" void plan_tuning_defaults(long long* out) {
    GemmTuning t;
    for (int i = 0; i < 13; ++i) out[i] = *fields(t, i);
}
// out: body, rows_main, pp_eligible, pp_tiles, pp_rounds, pp_rem, mb_main, then main and rest as
//      body, rows, nbm, nbn, ntiles, group_m, cf, tall, grid, rope_lut
extern "C" void plan_gemm(int bf16, int M, int N, int K, int epi_mask, int force_small_tile, int rope_lut, int rope_lut_bytes,
                          int co_streams, const long long* tuning, int* out) {
    GemmTuning t;
    for (int i = 0; i < 13; ++i) *fields(t, i) = tuning[i];
    GemmQuery q;
    q.bf16 = bf16 != 0; q.M = M; q.N = N; q.K = K; q.epi_mask = epi_mask; q.force_small_tile = force_small_tile != 0;
    q.rope_lut = rope_lut != 0; q.rope_lut_bytes = rope_lut_bytes; q.co_streams = co_streams;
    const GemmPlan p = cogs_plan_gemm(q, t);
    const int v[] = {p.body, p.rows_main, p.pp_eligible, p.pp_tiles, p.pp_rounds, p.pp_rem, p.mb_main};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    put(p.main, out + 7);
    put(p.rest, out + 17);
}
