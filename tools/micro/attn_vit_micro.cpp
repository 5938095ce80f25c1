// Stand-alone timing harness for csrc/attn_vit.hip (ViT block-diagonal attention, hd 72):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I cogstream_amd/csrc tools/micro/attn_vit_micro.cpp -o tools/micro/attn_vit_micro
//   attn_vit_micro [frames] [rows per frame] [layout: 0 token-major fused qkv, 1 head-major q | k | v] [attn_vit_len: 0 run-time end]
// The launch is the one cogs_plan_attention_vit (csrc/attn_plan.h) gives for the descriptor, as cogs_k_attention would take it.
#include "../../cogstream_amd/csrc/attn_vit.hip"
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <random>
int main(int argc, char** argv) {
    const int nseg = argc > 1 ? atoi(argv[1]) : 64, seg = argc > 2 ? atoi(argv[2]) : 924, heads = 16, hd = 72;
    const int hm = argc > 3 ? atoi(argv[3]) : 1;
    const long L = (long)nseg * seg, H = heads * hd;
    std::vector<uint16_t> h(L * 3 * H);
    std::mt19937 rng(1);
    std::normal_distribution<float> nd(0.f, 1.f);
    for (long i = 0; i < L; ++i)
        for (long c = 0; c < 3 * H; ++c) {
            float v = nd(rng) * (c < H ? 1.4426950408889634f / sqrtf(72.f) : 1.f);
            uint32_t u; std::memcpy(&u, &v, 4); h[i * 3 * H + c] = (uint16_t)((u + 0x7fff + ((u >> 16) & 1)) >> 16);
        }
    uint16_t *qkv, *out; int* cu;
    hipMalloc(&qkv, h.size() * 2); hipMalloc(&out, L * H * 2); hipMalloc(&cu, (nseg + 1) * 4);
    if (hm) {      // [row][q | k | v][head][hd] -> [q | k | v][head][row][hd]
        std::vector<uint16_t> t(h.size());
        for (long i = 0; i < L; ++i)
            for (int w = 0; w < 3; ++w)
                for (int hh = 0; hh < heads; ++hh)
                    std::memcpy(&t[((long)(w * heads + hh) * L + i) * hd], &h[i * 3 * H + w * H + hh * hd], hd * 2);
        h.swap(t);
    }
    hipMemcpy(qkv, h.data(), h.size() * 2, hipMemcpyHostToDevice);
    std::vector<int> hc(nseg + 1); for (int i = 0; i <= nseg; ++i) hc[i] = i * seg;
    hipMemcpy(cu, hc.data(), hc.size() * 4, hipMemcpyHostToDevice);
    CogsAttn a; a.dtype = COGS_DT_BF16; a.Q = qkv; a.K = qkv + H; a.V = qkv + 2 * H; a.O = out;
    a.ldq = a.ldk = a.ldv = 3 * H; a.ldo = H; a.cu_seqlens = cu; a.nseg = nseg; a.max_seqlen = seg;
    a.uniform_seqlen = seg;
    if (hm) {
        a.K = qkv + L * H; a.V = qkv + 2 * L * H; a.ldq = a.ldk = a.ldv = hd; a.head_stride = L * hd;
    }
    a.q_len = a.kv_len = (int)L; a.hq = a.hkv = heads; a.head_dim = hd; a.q_prescaled = 1;
    AttnTuning tuning;
    if (argc > 4) tuning.attn_vit_len = atoi(argv[4]);      // 0: the run-time-length kernel for every frame size
    AttnQuery q;
    q.head_dim = hd; q.q_len = q.kv_len = (int)L; q.hq = q.hkv = heads;
    q.ldq = a.ldq; q.ldk = a.ldk; q.ldv = a.ldv; q.ldo = a.ldo; q.head_stride = a.head_stride;
    q.has_cu = true; q.nseg = nseg; q.max_seqlen = seg; q.uniform_seqlen = seg; q.q_prescaled = 1;
    const AttnPlan plan = cogs_plan_attention_vit(q, tuning);
    if (plan.status != COGS_OK) { printf("plan rejected the descriptor: %d\n", plan.status); return 1; }
    printf("kernel %d, ragged end %d, grid (%d, %d, %d)\n", plan.kernel, plan.vit_end, plan.grid_x, plan.grid_y, plan.grid_z);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int i = 0; i < 3; ++i) cogs_k_attention_vit(0, a, plan);
    hipDeviceSynchronize();
    float best = 1e9f, sum = 0;
    for (int i = 0; i < 20; ++i) {
        hipEventRecord(e0, 0); cogs_k_attention_vit(0, a, plan); hipEventRecord(e1, 0); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1); best = ms < best ? ms : best; sum += ms;
    }
    const double fl = 4.0 * nseg * heads * (double)seg * seg * hd;
    printf("attn_vit %dx%d: mean %.4f ms min %.4f ms  %.1f TFLOP/s (min)\n", nseg, seg, sum / 20, best, fl / best / 1e9);
    return 0;
}
