// Host-side pieces shared by the C-ABI translation units (capi.hip, capi_vit.hip, capi_llm.hip): the handle, the
// per-launch profiling bracket, the pinned staging ring and the workspace carver. No kernel file includes this.
#pragma once
#include "../../include/cogs.h"
#include "common.h"
#include "kernels.h"
#include "debug.h"

#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>

struct cogs_ctx {
    int device = 0;
    // ViT
    bool vit_ok = false;
    cogs_vit_weights vit{};
    std::vector<cogs_vit_layer> vit_layers;
    float* vit_inv_freq = nullptr;  // device [head_dim/4]
    int vit_nfreq = 0;
    // projector
    bool proj_ok = false;
    cogs_proj_weights proj{};
    // LLM
    bool llm_ok = false;
    cogs_llm_weights llm{};
    std::vector<cogs_llm_layer> llm_layers;
    bool fp8_ok = false;            // cogs_llm_attach_fp8: e4m3 codes + row scales of the packed matrices
    cogs_llm_fp8_weights fp8{};
    std::vector<cogs_llm_fp8_layer> fp8_layers;
    float* llm_inv_freq = nullptr;  // device [head_dim/2]
    int llm_nfreq = 0; float llm_theta = 0.f;
    // pinned host staging for small host->device tables (segment boundaries): a ring of slots, each guarded by an
    // event recorded behind the copy that reads it, so a slot is never rewritten while a queued copy still needs it
    static constexpr int STAGE_SLOTS = 4;
    void* stage_host[STAGE_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    size_t stage_cap[STAGE_SLOTS] = {0, 0, 0, 0};
    hipEvent_t stage_ev[STAGE_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    bool stage_busy[STAGE_SLOTS] = {false, false, false, false};
    int stage_next = 0;
    // second stream of the frame-split encode (cogs_vit_encode): two halves of a small clip run side by side
    std::vector<hipStream_t> aux_streams;
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_joins;
    int vit_streams = 2;                  // cogs_vit_set_streams: 1 = never split
    // optional per-kernel-class event profiling (bench/roofline only)
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;      // pairs
    std::vector<int> prof_cls;
    std::vector<int> prof_n;              // kernels inside the bracket
    size_t prof_used = 0;
};

// RAII event bracket around one launch; a no-op unless cogs_profile_begin() was called
struct ProfScope {
    cogs_ctx* c; hipStream_t st; size_t slot = 0; bool on; long launches0 = 0;
    ProfScope(cogs_ctx* c_, hipStream_t st_, int cls) : c(c_), st(st_), on(c_->prof_on) {
        if (!on) return;
        launches0 = cogs_k_gemm_launch_count();
        if (c->prof_used * 2 + 2 > c->prof_ev.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            c->prof_ev.push_back(a); c->prof_ev.push_back(b);
        }
        slot = c->prof_used++;
        if (c->prof_cls.size() < c->prof_used) c->prof_cls.resize(c->prof_used);
        c->prof_cls[slot] = cls;
        (void)hipEventRecord(c->prof_ev[2 * slot], st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(c->prof_ev[2 * slot + 1], st);
        const long n = cogs_k_gemm_launch_count() - launches0;   // a GEMM bracket may hold two kernels (split)
        if (c->prof_n.size() < c->prof_used) c->prof_n.resize(c->prof_used);
        c->prof_n[slot] = n > 0 ? (int)n : 1;
    }
};
#define PROF(cls) ProfScope _prof_scope(h, st, cls)

#define COGS_TRY(x)                      \
    do {                                 \
        const int _rc = (x);             \
        if (_rc != COGS_OK) return _rc;  \
    } while (0)

#define COGS_INTERNAL __attribute__((visibility("hidden")))      // shared between the capi*.hip files, not exported
// copy `bytes` of host data to the device on `st` through the handle's pinned ring (no stream synchronisation); capi.hip
COGS_INTERNAL int stage_h2d(cogs_ctx* c, hipStream_t st, void* dst, const void* src, size_t bytes);

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
inline int esize(int dtype) { return dtype == COGS_DT_BF16 ? 2 : 4; }

// Hands out consecutive 256-byte aligned pieces of a workspace. Every scratch layout is ONE function that fills a struct of
// named pointers from a Carver; a null base gives null pointers and the size: query and carve cannot disagree.
struct Carver {
    char* base; size_t off = 0;
    explicit Carver(void* p) : base((char*)p) {}
    void* take(size_t bytes) { const size_t o = off; off = align_up(off + bytes); return base ? base + o : nullptr; }
};

// workspace of a log-sum-exp walk (cogs_row_lse; with the logits panel: cogs_lm_score), part: null without a column split; capi.hip
struct LseScratch { void *state, *part; float* panel; size_t bytes; };
COGS_INTERNAL LseScratch lse_scratch(const CogsLsePlan& p, bool with_panel, void* base);
COGS_INTERNAL void lse_report(const CogsLsePlan& p);      // the plan into the lm_score_last_* read-only switches
