// common.h -- shared host-side plumbing of libmapf_gpt_amd.so (error strings, HIP checks,
// per-kernel-class event timing).  gfx950 only; no CUDA compatibility layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/mapf_gpt_amd.h"
#include "device_mem.h"

namespace mgpt {

void set_error(const char *fmt, ...);

// Allocation generation, PER CONTEXT: a policy / env context bumps its own counter whenever it frees or re-allocates device
// memory that a captured step graph may have baked in (weight planes and workspaces at finalize / lazy mode build, lifelong
// goal queues).  mgpt_step compares the generations of the contexts IT holds with the values it saw at its last step and, on
// a change, drops its graph and runs one eager step first; other models, envs and runners of the process are not disturbed.
// (The tokenizer context never re-allocates after create.)
uint64_t gpt_generation(const mgpt_gpt *g);
uint64_t env_generation(const mgpt_env *e);
// instances and agents per instance of an env context (step.hip sizes its live list and compact buffers from them)
void env_shape(const mgpt_env *e, int *n_inst, int *n_agents);
// max_episode_steps of an env context (step.hip sizes the episode recorder's buffers from it)
int env_max_steps(const mgpt_env *e);
// rule mask, lifelong flag and frame of an env context; the device state a tokenizer context lends to the expert (expert.hip)
void env_config(const mgpt_env *e, int *H, int *W, int *n_grids, int *rules, int *lifelong);
struct TokView {
    const uint16_t *dist;
    const uint8_t *grids;
    int n_inst, n_agents, H, W, n_grids;
    bool have_agents;
};
void tok_view(const mgpt_tokenizer *t, TokView *out);
// expert.hip: the contexts an expert was made from and whether it is in shield mode (step.hip: mgpt_step_set_shield)
void expert_contexts(const mgpt_expert *ex, const mgpt_tokenizer **tok, const mgpt_env **env, bool *shield);
// gpt.hip: the sampler on the compact logits of the live instances (sample_live_kernel), for step.hip's retire mode
int sample_actions_live(const float *d_logits, const int32_t *d_live, const int32_t *d_count, int n_agents, int n_inst, int64_t grid_rows,
                        int32_t *d_actions, int do_sample, uint64_t seed, uint64_t step, const uint64_t *d_step, uint64_t row0, hipStream_t s);

#define MGPT_HIP(call)                                                                     \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess) {                                                           \
            mgpt::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
            return MGPT_ERR_HIP;                                                           \
        }                                                                                  \
    } while (0)

#define MGPT_REQUIRE(cond, code, ...)                                                      \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            mgpt::set_error(__VA_ARGS__);                                                  \
            return (code);                                                                 \
        }                                                                                  \
    } while (0)

#define MGPT_LAUNCH_CHECK()                                                                \
    do {                                                                                   \
        hipError_t e__ = hipGetLastError();                                                \
        if (e__ != hipSuccess) {                                                           \
            mgpt::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__), __FILE__, __LINE__); \
            return MGPT_ERR_HIP;                                                           \
        }                                                                                  \
    } while (0)

// kernel classes for the timing hooks (names in prof.cpp)
enum ProfId {
    P_BFS = 0, P_TOK_UPDATE, P_TOK_NEXT, P_TOKENS, P_ENV_STEP, P_ENV_METRICS,
    P_EMBED, P_LAYERNORM, P_GEMM_QKV, P_ATTN, P_GEMM_PROJ, P_GEMM_FC, P_GEMM_PROJ2, P_MLP_FUSED,
    P_HEAD, P_SAMPLE, P_PACK, P_LNQKV_FUSED,
    P_ATTN_LAST, P_GEMM_PROJ_LAST, P_MLP_FUSED_LAST,    // the last layer's launches (token 255 only, model.py:186): timed apart from the full ones
    P_HEAD_SEQ, P_SCORE,                                // ln_f + head + cross-entropy of every position (mgpt_gpt_forward_seq), last-position scoring
    P_DS_HASH, P_DS_INSERT, P_DS_CLASSIFY, P_DS_RESOLVE, P_DS_BALANCE, P_DS_SELECT, P_DS_GATHER,   // dataset builder (dataset_build.hip)
    P_EXPERT_PLAN,                                      // the PIBT expert's plan kernel (expert.hip)
    P_EXPERT_SEARCH,                                    // the LaCAM search kernel, every launch of a solve (expert.hip)
    P_EXPERT_CELL_DEGREE,                               // the swap rule's degree map, once per context (expert.hip)
    P_EXPERT_REFINE_PATH, P_EXPERT_REFINE_ROUND, P_EXPERT_REFINE_FINAL,   // the refinement pass of a solve: path, every round, final (expert.hip)
    P_EXPERT_LIFELONG_POST,                             // lifelong episodes: arrivals, since and the arrivals log after the env step (expert.hip)
    P_EXPERT_SHIELD,                                    // the collision shield's plan kernel (expert.hip)
    P_STEP_RECORD,                                      // the episode recorder's store of a step (step.hip)
    P_DS_PATHS, P_DS_EPISODE_TOKENS,                    // batched episode tokenizer: paths + labels + records, rows (tokenizer.hip)
    P_DS_PATHS_LIFELONG, P_DS_EPISODE_TOKENS_LIFELONG,  // the same for lifelong logs: a goal per timestep (tokenizer.hip)
    P_EXPERT_SHIELD_LIFELONG_POST,                      // the shield on lifelong episodes: since and the arrivals log after the env step (expert.hip)
    P_COUNT
};

// RAII: records start/stop events around a launch when profiling is enabled (no-op otherwise)
struct ProfScope {
    int slot;
    hipStream_t s;
    ProfScope(ProfId id, hipStream_t stream);
    ~ProfScope();
};

// raises a kernel's limit of dynamic LDS (a per-device function attribute) to `bytes`
template <class K>
inline hipError_t set_max_lds(K *kernel, int bytes)
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace mgpt
