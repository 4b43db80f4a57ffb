// step.hip -- one whole environment step behind ONE entry point, replayed as a hipGraph:
//     tokenizer.update_agents(pos, goal, last_actions)   observation_generator.cpp:432-485
//     tokens  = tokenizer.generate_observations()        observation_generator.cpp:516-528
//     actions = policy.act(tokens)                       model.py:244-260
//     env.step(actions)                                  create_env.py:14-15
// (the loop of inference.py:151-172 + example.py:63-65).  The launch sequence of a step is static -- every data-dependent
// decision (dirty-flag BFS, done instances, rescale branches) lives inside the kernels -- so after one eager step (which
// builds the lazily packed weight planes) the sequence is captured once and replayed; the only per-step scalar, the RNG
// step counter, lives in device memory and is bumped by the graph's last node.  For small workloads (one 32-agent env:
// ~40 launches of a few microseconds each) this removes the per-launch host cost and the Python/ctypes round trips.
//
// Retire mode (mgpt_step_set_retire): the reference's run_episode leaves an episode once all agents are terminated or truncated
// (create_env.py:15-18); a batch cannot leave, but it can stop forwarding the finished instances.  A poll compacts the ids of the
// instances with done == 0 into an ordered live list (live_list_kernel) and reads the count back -- the only host synchronisation of the
// mode.  Between polls the list is frozen: the tokenizer still runs over all rows, the token rows of the live instances are gathered
// into a compact buffer, the policy forwards those rows alone, and sample_live_kernel (gpt.hip) writes each action to its global row
// with the draw keyed by that global row.  An instance that finishes inside the window is forwarded until the next poll; the env
// ignores it (env.hip: env_step_kernel returns on done != 0).  Eager launches only: the row count changes from poll to poll.
//
// Recording (mgpt_step_set_record): one more launch per step, record_kernel, after the env step and before the
// counter bump, stores every row's new position and the action the env was handed into per-step slots of two trajectory buffers.  The
// slot index is read on the device (step counter minus the counter at reset), so the launch is static and a captured graph replays it.
#include <vector>

#include "common.h"

namespace mgpt {
bool prof_is_enabled();
}
using namespace mgpt;

// internal entry of gpt.hip: mgpt_gpt_act with the RNG step read from device memory
extern "C" int mgpt_gpt_act_dev(mgpt_gpt *g, const uint8_t *d_tokens, int rows, int32_t *d_actions, float *d_logits, int do_sample,
                                uint64_t seed, const uint64_t *d_step, uint64_t row0, int precision, void *stream);

struct mgpt_step {
    mgpt_tokenizer *tok = nullptr;
    mgpt_gpt *gpt = nullptr;
    mgpt_env *env = nullptr;
    int rows = 0, precision = 0, do_sample = 0;
    uint64_t seed = 0, row0 = 0;
    uint64_t *d_step = nullptr;                 // device: RNG step counter (model.py:257's generator state, in our counter form)
    const int16_t *d_pos = nullptr, *d_goal = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t cap_stream = nullptr;           // capture happens here (the caller's stream may be the NULL stream, which cannot capture)
    int eager_runs = 0;
    // what the captured graph was recorded with
    const uint8_t *cap_tokens = nullptr;
    const int32_t *cap_actions = nullptr;
    int cap_gmc = -1;
    bool capture_failed = false;
    uint64_t seen_gpt_gen = 0, seen_env_gen = 0; // generations of OUR contexts after our last step (0: never ran)
    // retire mode (all NULL / 0 when off)
    bool retire = false;
    int n_inst = 0, n_agents = 0;
    int n_live = 0;                             // live instances at the last poll (host copy: sizes the forward until the next poll)
    struct Retire {                             // owned by retire_mem
        int32_t *d_live = nullptr;              // [n_inst] ids of the live instances, ascending; -1 beyond the count
        int32_t *d_count = nullptr;             // device copy of n_live
        int32_t *h_count = nullptr;             // pinned: the poll's read-back
        uint8_t *d_ctokens = nullptr;           // [rows][256] token rows of the live instances, compact
        float *d_clogits = nullptr;             // [rows][67] their logits
    } rt;
    // collision shield (mgpt_step_set_shield): NULL when off
    mgpt_expert *shield = nullptr;              // a shield-mode expert over tok and env, owned by the caller
    float *d_logits = nullptr;                  // [rows][67] the plain path's logits of the last step (retire mode has rt.d_clogits)
    // episode recorder (mgpt_step_set_record): all NULL / 0 when off
    struct Record {                             // owned by record_mem
        uint32_t *d_pos = nullptr;              // [T + 1][rows] one (row, col) int16 pair per word: slot 0 = the reset positions, slot t + 1 after step t
        int8_t *d_act = nullptr;                // [T][rows] the action handed to the env at step t
        uint64_t *d_t0 = nullptr;               // the step counter at the last reset: slot index = *d_step - *d_t0
        int T = 0;                              // the env's max_episode_steps
    } rec;
    DeviceArena mem, retire_mem, shield_mem, record_mem;    // d_step; rt; d_logits; rec
};

namespace {
__global__ void bump_kernel(uint64_t *ctr) { *ctr += 1; }
__global__ void set_kernel(uint64_t *ctr, uint64_t v) { *ctr = v; }

// One step of the episode recorder: row's cell after the env step -> traj_pos[t + 1][row] (one 4-byte store), the action the env was
// handed -> traj_act[t][row], with t = *d_step - *t0 read here, so the launch has no per-step argument.  Steps beyond the buffers'
// T slots (and a counter behind t0: the unsigned difference is then huge) write nothing.  Every row is handled, done instances too:
// they do not move, and their entries beyond the episode's length mean nothing.
__global__ __launch_bounds__(256) void record_kernel(const uint32_t *__restrict__ pos, const int32_t *__restrict__ actions,
                                                     const uint64_t *__restrict__ d_step, const uint64_t *__restrict__ t0, int T, int rows,
                                                     uint32_t *__restrict__ traj_pos, int8_t *__restrict__ traj_act)
{
    const uint64_t t = *d_step - *t0;
    if (t >= (uint64_t)T) return;
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    traj_pos[(t + 1) * (uint64_t)rows + row] = pos[row];
    traj_act[t * (uint64_t)rows + row] = (int8_t)actions[row];
}

constexpr int kLiveThreads = 1024, kLiveWaves = kLiveThreads / 64;

// Stable stream compaction of the instances with done == 0: live[0 .. count) = their ids in ascending order, live[count .. n_inst) = -1.
// ONE workgroup walks n_inst in passes of kLiveThreads flags (a batch has at most 65536 instances: 64 passes).  Inside a wave the rank of
// a live lane is the population count of the ballot below it; across the waves of a pass the wave totals go through LDS and every thread
// sums the ones before its wave; across passes a running total that all threads carry.  Every slot is a function of the flags alone --
// no atomics -- so the same flags give the same bits.
__global__ __launch_bounds__(kLiveThreads) void live_list_kernel(const uint8_t *__restrict__ done, int n_inst, int32_t *__restrict__ live,
                                                                 int32_t *__restrict__ count)
{
    __shared__ int wave_total[kLiveWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int running = 0;                                            // live instances of the passes so far (workgroup-uniform)
    for (int base = 0; base < n_inst; base += kLiveThreads) {   // (uniform trip count: every thread reaches both barriers)
        const int i = base + tid;
        const bool is_live = i < n_inst && done[i] == 0;
        const unsigned long long mask = __ballot(is_live);      // 64-bit on a wave64 target
        const int rank = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kLiveWaves; w++) {
            const int t = wave_total[w];
            total += t;
            if (w < wave) before += t;
        }
        if (is_live) live[running + before + rank] = i;         // < running + total <= n_inst
        running += total;
        __syncthreads();                                        // wave_total is rewritten by the next pass
    }
    for (int i = running + tid; i < n_inst; i += kLiveThreads) live[i] = -1;
    if (tid == 0) *count = running;
}

__global__ void live_all_kernel(int32_t *__restrict__ live, int32_t *__restrict__ count, int n_inst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_inst) live[i] = i;
    if (i == 0) *count = n_inst;
}

// Token rows (256 B = 16 x uint4) of the live instances -> compact rows: compact row j = instance live[j / n_agents], agent j % n_agents.
// 16 lanes per row, one 16-byte load and store each.  The row count comes from device memory (*d_count instances); threads beyond it,
// and rows whose id is not an instance, do nothing.
__global__ __launch_bounds__(256) void gather_live_rows_kernel(const uint4 *__restrict__ tokens, const int32_t *__restrict__ live,
                                                               const int32_t *__restrict__ d_count, int n_agents, int n_inst,
                                                               uint4 *__restrict__ out)
{
    const int64_t n = (int64_t)min(max(*d_count, 0), n_inst) * n_agents;
    const int64_t j = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (j >= n) return;
    const int inst = live[j / n_agents];
    if (inst < 0 || inst >= n_inst) return;
    const int64_t src = (int64_t)inst * n_agents + (int)(j % n_agents);
    const int q = threadIdx.x & 15;
    out[j * 16 + q] = tokens[src * 16 + q];
}

int launch_live_list(const uint8_t *d_done, int n_inst, int32_t *d_live, int32_t *d_count, hipStream_t s)
{
    hipLaunchKernelGGL(live_list_kernel, dim3(1), dim3(kLiveThreads), 0, s, d_done, n_inst, d_live, d_count);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// the policy part of a retire-mode step: gather -> forward on the compact rows -> sample into the global rows
int act_live(mgpt_step *st, const uint8_t *d_tokens, int32_t *d_actions, hipStream_t s)
{
    if (st->n_live == 0) return MGPT_OK;
    const int live_rows = st->n_live * st->n_agents;
    hipLaunchKernelGGL(gather_live_rows_kernel, dim3(cdiv(live_rows, 16)), dim3(256), 0, s, (const uint4 *)d_tokens, st->rt.d_live, st->rt.d_count,
                       st->n_agents, st->n_inst, (uint4 *)st->rt.d_ctokens);
    MGPT_LAUNCH_CHECK();
    int rc = mgpt_gpt_forward(st->gpt, st->rt.d_ctokens, live_rows, st->rt.d_clogits, st->precision, s);
    if (rc != MGPT_OK) return rc;
    return sample_actions_live(st->rt.d_clogits, st->rt.d_live, st->rt.d_count, st->n_agents, st->n_inst, live_rows, d_actions, st->do_sample, st->seed, 0,
                               st->d_step, st->row0, s);
}

void free_record(mgpt_step *st)
{
    st->record_mem.release();
    st->rec = mgpt_step::Record();
}

void free_retire(mgpt_step *st)
{
    st->retire_mem.release();
    st->rt = mgpt_step::Retire();
    st->retire = false; st->n_live = 0;
}

int step_body(mgpt_step *st, uint8_t *d_tokens, int32_t *d_actions, int gmc, hipStream_t s)
{
    int rc;
    if ((rc = mgpt_tokenizer_update_agents(st->tok, st->d_pos, st->d_goal, d_actions, gmc, s)) != MGPT_OK) return rc;
    if ((rc = mgpt_tokenizer_generate_observations(st->tok, d_tokens, s)) != MGPT_OK) return rc;
    if (st->retire) {
        if ((rc = act_live(st, d_tokens, d_actions, s)) != MGPT_OK) return rc;
    } else if ((rc = mgpt_gpt_act_dev(st->gpt, d_tokens, st->rows, d_actions, st->d_logits, st->do_sample, st->seed, st->d_step, st->row0, st->precision,
                               s)) != MGPT_OK)
        return rc;
    if (st->shield) {                                           // the sampled actions become every agent's first candidate of a PIBT step
        if (st->retire) {
            if (st->n_live > 0 && (rc = mgpt_expert_shield(st->shield, st->rt.d_clogits, MGPT_VOCAB, st->rt.d_live, st->rt.d_count, d_actions, s)) != MGPT_OK)
                return rc;
        } else if ((rc = mgpt_expert_shield(st->shield, st->d_logits, MGPT_VOCAB, nullptr, nullptr, d_actions, s)) != MGPT_OK)
            return rc;
    }
    if ((rc = mgpt_env_step(st->env, d_actions, s)) != MGPT_OK) return rc;
    if (st->shield && (rc = mgpt_expert_shield_commit(st->shield, s)) != MGPT_OK) return rc;
    if (st->rec.d_pos) {
        ProfScope prof(P_STEP_RECORD, s);
        hipLaunchKernelGGL(record_kernel, dim3(cdiv(st->rows, 256)), dim3(256), 0, s, (const uint32_t *)st->d_pos, d_actions, st->d_step, st->rec.d_t0,
                           st->rec.T, st->rows, st->rec.d_pos, st->rec.d_act);
        MGPT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(bump_kernel, dim3(1), dim3(1), 0, s, st->d_step);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

void drop_graph(mgpt_step *st)
{
    if (st->exec) (void)hipGraphExecDestroy(st->exec);
    if (st->graph) (void)hipGraphDestroy(st->graph);
    st->exec = nullptr; st->graph = nullptr;
}
}  // namespace

extern "C" int mgpt_step_create(mgpt_step **out, mgpt_tokenizer *tok, mgpt_gpt *gpt, mgpt_env *env, int rows, int precision,
                                int do_sample, uint64_t seed, uint64_t row0)
{
    MGPT_REQUIRE(out && tok && gpt && env && rows > 0, MGPT_ERR_ARG, "bad argument");
    {   // a tokenizer with a larger value limit than the policy's vocabulary was built for emits ids the embedding does not have (the reference:
        // IndexError in nn.Embedding, model.py:126,172)
        int vocab = 0;
        const int rc = mgpt_tokenizer_vocab_size(tok, &vocab);
        if (rc != MGPT_OK) return rc;
        MGPT_REQUIRE(vocab <= MGPT_VOCAB, MGPT_ERR_UNSUPPORTED, "the tokenizer's vocabulary has %d tokens (cost2go_value_limit %d), the policy's embedding %d",
                     vocab, (vocab - 27) / 2, MGPT_VOCAB);
    }
    mgpt_step *st = new mgpt_step();
    st->tok = tok; st->gpt = gpt; st->env = env; st->rows = rows; st->precision = precision; st->do_sample = do_sample;
    st->seed = seed; st->row0 = row0;
    int rc = mgpt_env_state(env, &st->d_pos, &st->d_goal, nullptr);
    if (rc != MGPT_OK) { delete st; return rc; }
    hipError_t e = st->mem.alloc(&st->d_step, sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemset(st->d_step, 0, sizeof(uint64_t));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st->cap_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_error("device allocation / hipStreamCreate failed in mgpt_step_create: %s", hipGetErrorString(e));
        delete st;
        return MGPT_ERR_HIP;
    }
    *out = st;
    return MGPT_OK;
}

extern "C" int mgpt_step_destroy(mgpt_step *st)
{
    if (!st) return MGPT_OK;
    drop_graph(st);
    free_retire(st);
    free_record(st);
    if (st->cap_stream) (void)hipStreamDestroy(st->cap_stream);
    delete st;
    return MGPT_OK;
}

extern "C" int mgpt_step_reset(mgpt_step *st, uint64_t step0, void *stream)
{
    MGPT_REQUIRE(st, MGPT_ERR_ARG, "NULL argument");
    drop_graph(st);          // between episodes the contexts may re-allocate (lifelong goal queues): next run re-captures
    hipLaunchKernelGGL(set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, st->d_step, step0);
    MGPT_LAUNCH_CHECK();
    if (st->retire) {        // a new episode: every instance is live until the next poll says otherwise
        hipLaunchKernelGGL(live_all_kernel, dim3(cdiv(st->n_inst, 256)), dim3(256), 0, (hipStream_t)stream, st->rt.d_live, st->rt.d_count, st->n_inst);
        MGPT_LAUNCH_CHECK();
        st->n_live = st->n_inst;
    }
    if (st->rec.d_pos) {     // a new recording: slot index 0 at step0, empty buffers, the env's (already reset) positions in slot 0
        hipStream_t s = (hipStream_t)stream;
        const size_t rows = (size_t)st->rows;
        hipLaunchKernelGGL(set_kernel, dim3(1), dim3(1), 0, s, st->rec.d_t0, step0);
        MGPT_LAUNCH_CHECK();
        MGPT_HIP(hipMemsetAsync(st->rec.d_pos, 0, ((size_t)st->rec.T + 1) * rows * sizeof(uint32_t), s));
        MGPT_HIP(hipMemsetAsync(st->rec.d_act, 0, (size_t)st->rec.T * rows, s));
        MGPT_HIP(hipMemcpyAsync(st->rec.d_pos, st->d_pos, rows * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    }
    return MGPT_OK;
}

extern "C" int mgpt_step_set_record(mgpt_step *st, int enable)
{
    MGPT_REQUIRE(st, MGPT_ERR_ARG, "NULL argument");
    drop_graph(st);                               // the launch sequence changes either way
    if (!enable) {
        free_record(st);                          // (freeing waits for the work that still writes the buffers)
        return MGPT_OK;
    }
    if (st->rec.d_pos) return MGPT_OK;
    const int T = env_max_steps(st->env);
    const size_t rows = (size_t)st->rows;
    DeviceArena &rm = st->record_mem;
    hipError_t e = rm.alloc(&st->rec.d_pos, ((size_t)T + 1) * rows * sizeof(uint32_t));
    if (e == hipSuccess) e = rm.alloc(&st->rec.d_act, (size_t)T * rows);
    if (e == hipSuccess) e = rm.alloc(&st->rec.d_t0, sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemset(st->rec.d_pos, 0, ((size_t)T + 1) * rows * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(st->rec.d_act, 0, (size_t)T * rows);
    if (e == hipSuccess) e = hipMemcpy(st->rec.d_t0, st->d_step, sizeof(uint64_t), hipMemcpyDeviceToDevice);   // recording starts at slot 0 from here
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("allocation failed in mgpt_step_set_record: %s", hipGetErrorString(e));
        free_record(st);
        return MGPT_ERR_HIP;
    }
    st->rec.T = T;
    return MGPT_OK;
}

extern "C" int mgpt_step_copy_record(mgpt_step *st, int16_t *d_pos_out, int8_t *d_act_out, void *stream)
{
    MGPT_REQUIRE(st, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(st->rec.d_pos, MGPT_ERR_STATE, "recording is off (mgpt_step_set_record)");
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)st->rows;
    if (d_pos_out) MGPT_HIP(hipMemcpyAsync(d_pos_out, st->rec.d_pos, ((size_t)st->rec.T + 1) * rows * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    if (d_act_out) MGPT_HIP(hipMemcpyAsync(d_act_out, st->rec.d_act, (size_t)st->rec.T * rows, hipMemcpyDeviceToDevice, s));
    return MGPT_OK;
}

extern "C" int mgpt_step_set_retire(mgpt_step *st, int enable)
{
    MGPT_REQUIRE(st, MGPT_ERR_ARG, "NULL argument");
    if (!enable) {
        if (st->retire) free_retire(st);          // (freeing waits for the work that still reads the buffers)
        return MGPT_OK;
    }
    if (st->retire) return MGPT_OK;
    drop_graph(st);
    env_shape(st->env, &st->n_inst, &st->n_agents);
    MGPT_REQUIRE((int64_t)st->n_inst * st->n_agents == st->rows, MGPT_ERR_ARG, "the step has %d rows, its env %d x %d", st->rows, st->n_inst,
                 st->n_agents);
    DeviceArena &rm = st->retire_mem;
    hipError_t e = rm.alloc(&st->rt.d_live, (size_t)st->n_inst * sizeof(int32_t));
    if (e == hipSuccess) e = rm.alloc(&st->rt.d_count, sizeof(int32_t));
    if (e == hipSuccess) e = rm.alloc_host(&st->rt.h_count, sizeof(int32_t));
    if (e == hipSuccess) e = rm.alloc(&st->rt.d_ctokens, (size_t)st->rows * MGPT_CONTEXT);
    if (e == hipSuccess) e = rm.alloc(&st->rt.d_clogits, (size_t)st->rows * MGPT_VOCAB * sizeof(float));
    if (e == hipSuccess) {                        // all live, as after mgpt_step_reset
        std::vector<int32_t> ids((size_t)st->n_inst);
        for (int i = 0; i < st->n_inst; i++) ids[(size_t)i] = i;
        e = hipMemcpy(st->rt.d_live, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(st->rt.d_count, &st->n_inst, sizeof(int32_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        set_error("allocation failed in mgpt_step_set_retire: %s", hipGetErrorString(e));
        free_retire(st);
        return MGPT_ERR_HIP;
    }
    st->retire = true;
    st->n_live = st->n_inst;
    return MGPT_OK;
}

extern "C" int mgpt_step_set_shield(mgpt_step *st, mgpt_expert *ex)
{
    MGPT_REQUIRE(st, MGPT_ERR_ARG, "NULL argument");
    drop_graph(st);
    if (!ex) {
        st->shield = nullptr;
        st->shield_mem.release();                 // (freeing waits for the work that still reads the buffer)
        st->d_logits = nullptr;
        return MGPT_OK;
    }
    const mgpt_tokenizer *tok = nullptr;
    const mgpt_env *env = nullptr;
    bool on = false;
    expert_contexts(ex, &tok, &env, &on);
    MGPT_REQUIRE(tok == st->tok && env == st->env, MGPT_ERR_ARG, "the expert was made from another tokenizer or env context than this step");
    MGPT_REQUIRE(on, MGPT_ERR_STATE, "mgpt_expert_set_shield(ex, 1) must precede mgpt_step_set_shield");
    if (!st->d_logits) {
        const hipError_t e = st->shield_mem.alloc(&st->d_logits, (size_t)st->rows * MGPT_VOCAB * sizeof(float));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("allocation failed in mgpt_step_set_shield: %s", hipGetErrorString(e));
            st->d_logits = nullptr;
            return MGPT_ERR_HIP;
        }
    }
    st->shield = ex;
    return MGPT_OK;
}

extern "C" int mgpt_step_copy_shield_logits(mgpt_step *st, float *d_out, void *stream)
{
    MGPT_REQUIRE(st && d_out, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(st->shield && st->d_logits, MGPT_ERR_STATE, "no shield is attached (mgpt_step_set_shield)");
    MGPT_HIP(hipMemcpyAsync(d_out, st->d_logits, (size_t)st->rows * MGPT_VOCAB * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGPT_OK;
}

extern "C" int mgpt_step_poll_live(mgpt_step *st, int *n_live, void *stream)
{
    MGPT_REQUIRE(st, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(st->retire, MGPT_ERR_STATE, "mgpt_step_set_retire(step, 1) must precede mgpt_step_poll_live");
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *d_done = nullptr;
    int rc = mgpt_env_state(st->env, nullptr, nullptr, &d_done);
    if (rc != MGPT_OK) return rc;
    if ((rc = launch_live_list(d_done, st->n_inst, st->rt.d_live, st->rt.d_count, s)) != MGPT_OK) return rc;
    MGPT_HIP(hipMemcpyAsync(st->rt.h_count, st->rt.d_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MGPT_HIP(hipStreamSynchronize(s));
    st->n_live = *st->rt.h_count;
    MGPT_REQUIRE(st->n_live >= 0 && st->n_live <= st->n_inst, MGPT_ERR_STATE, "live count %d outside 0 .. %d", st->n_live, st->n_inst);
    if (n_live) *n_live = st->n_live;
    return MGPT_OK;
}

extern "C" int mgpt_step_copy_live(mgpt_step *st, int32_t *d_live_out, float *d_logits_out, void *stream)
{
    MGPT_REQUIRE(st, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(st->retire, MGPT_ERR_STATE, "retire mode is off");
    hipStream_t s = (hipStream_t)stream;
    if (d_live_out) MGPT_HIP(hipMemcpyAsync(d_live_out, st->rt.d_live, (size_t)st->n_inst * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (d_logits_out)
        MGPT_HIP(hipMemcpyAsync(d_logits_out, st->rt.d_clogits, (size_t)st->rows * MGPT_VOCAB * sizeof(float), hipMemcpyDeviceToDevice, s));
    return MGPT_OK;
}

extern "C" int mgpt_live_list(const uint8_t *d_done, int n_inst, int32_t *d_live, int32_t *d_count, void *stream)
{
    MGPT_REQUIRE(d_done && d_live && d_count && n_inst > 0, MGPT_ERR_ARG, "bad argument");
    return launch_live_list(d_done, n_inst, d_live, d_count, (hipStream_t)stream);
}

extern "C" int mgpt_step_run(mgpt_step *st, uint8_t *d_tokens, int32_t *d_actions, int goals_may_change, int use_graph, void *stream)
{
    MGPT_REQUIRE(st && d_tokens && d_actions, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(!(st->retire && use_graph), MGPT_ERR_UNSUPPORTED,
                 "retire mode runs eager launches only (use_graph = 0): the policy's row count changes from poll to poll");
    MGPT_REQUIRE(!st->retire || ((uintptr_t)d_tokens & 15) == 0, MGPT_ERR_ARG, "retire mode gathers 16-byte vectors: d_tokens must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int gmc = goals_may_change ? 1 : 0;
    // one of OUR contexts re-allocated or freed device memory since our last step (weights reloaded -> planes freed and rebuilt lazily,
    // goal queues replaced): the graph holds dead pointers, and the rebuild (allocations, synchronous copies, null-stream pack
    // kernels) must not happen inside a capture -> drop the graph and run one eager step first
    if (gpt_generation(st->gpt) != st->seen_gpt_gen || env_generation(st->env) != st->seen_env_gen) {
        drop_graph(st);
        st->eager_runs = 0;
    }
    // eager: first step (lazy weight-plane build allocates), timing hooks on (their events belong to the eager stream), opt-out
    if (!use_graph || st->capture_failed || st->eager_runs < 1 || prof_is_enabled()) {
        st->eager_runs++;
        const int rc = step_body(st, d_tokens, d_actions, gmc, s);
        st->seen_gpt_gen = gpt_generation(st->gpt);   // (the lazy build inside this step bumped it)
        st->seen_env_gen = env_generation(st->env);
        return rc;
    }
    if (!st->exec || st->cap_tokens != d_tokens || st->cap_actions != d_actions || st->cap_gmc != gmc) {
        drop_graph(st);
        hipError_t e = hipStreamBeginCapture(st->cap_stream, hipStreamCaptureModeRelaxed);
        int rc = MGPT_OK;
        if (e == hipSuccess) {
            rc = step_body(st, d_tokens, d_actions, gmc, st->cap_stream);   // recorded, not executed
            e = hipStreamEndCapture(st->cap_stream, &st->graph);
        }
        if (e == hipSuccess && rc == MGPT_OK) e = hipGraphInstantiate(&st->exec, st->graph, nullptr, nullptr, 0);
        if (e != hipSuccess || rc != MGPT_OK) {          // fall back to eager launches for good; nothing has run yet for this step
            (void)hipGetLastError();
            drop_graph(st);
            st->capture_failed = true;
            return step_body(st, d_tokens, d_actions, gmc, s);
        }
        st->cap_tokens = d_tokens; st->cap_actions = d_actions; st->cap_gmc = gmc;
    }
    MGPT_HIP(hipGraphLaunch(st->exec, s));
    return MGPT_OK;
}
