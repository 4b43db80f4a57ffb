// expert.hip -- a device-resident PIBT expert (priority inheritance with backtracking): the role of run_expert() in the reference's
// dataset/generate_dataset.py:214-230 and of its logging environment (experiment_setup/create_env.py:8-33, LogActions :49-60).
//
// The reference's expert is LaCAM3 under POGEMA, neither of which is in its tree.  What is built here is the configuration generator
// of such a search, one step at a time, by this project's own spec -- a weaker teacher than LaCAM: nothing
// guarantees that all agents stand on their goals at once.
//
// One step of one instance:
//   order      agents by (since desc, id asc), since = steps since the agent last stood on its goal;
//   candidates of agent a: the cells pos[a] + move[k], k = 0..4 (env.hip's action numbering), not blocked and reachable from a's goal,
//              tried by ascending key (((d * 2 + o) * 32 + r_k) * 8 + k): d = a's BFS distance-to-goal at the cell (the tokenizer's field),
//              o = another agent stands there now, r_k = bits [5k, 5k + 5) of the sampler's splitmix value for (seed, t, global row);
//   PIBT(a, parent): take the first candidate u that is not reserved, is not the parent's cell and is not a swap with a decided agent;
//              reserve it; if an undecided agent c stands on u, PIBT(c, a) -- when that fails, c has taken u for itself and a goes on to
//              its next candidate.  With no candidate left a stays (taking its own cell back from the parent) and reports failure.
//
// One wave64 workgroup per instance.  The recursion is an explicit stack in dynamic LDS (8 bytes per frame, depth <= n_agents, sized
// from n_agents at launch); its control flow is wave-uniform: every lane runs the same serial program on the same addresses, so a
// lane only ever reads back what it stored itself and the serial part needs no barrier.  The lanes help where there is width: the
// priority rank is a counting sort in strided loops, occupancy is scattered (and cleared again by scattering NIL at the end of the
// kernel, never by a whole-grid clear), and the five candidate keys of an agent are formed by five lanes, one dist load each, and ranked
// with shuffles.  occ_now / next_occ are u16 agent ids (NIL = 0xFFFF) in a global workspace [n_inst][2][H*W]: one code path for every
// map size.  Every write is a plain vector store; no atomics.  The kernel is latency-bound pointer chasing (a chain of dependent
// loads of a few bytes), not bandwidth- or ALU-bound.
#include "common.h"

using namespace mgpt;

namespace {

constexpr unsigned kNil = 0xFFFFu;
constexpr unsigned kUnreach = 65535u;       // tokenizer.hip: wall / unreached in a distance field

// the sampler's splitmix arithmetic (gpt.hip: uniform01) before its final shift
__device__ __forceinline__ uint64_t splitmix_z(uint64_t seed, uint64_t step, uint64_t row)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (step + 1ull);
    z ^= row * 0xD1342543DE82EF95ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// frame word y: sorted candidate actions, 3 bits each, in bits [0, 15); their count in [15, 18); the next one to try in [18, 21);
// bit 21: a child call is outstanding
constexpr unsigned kFrameWaiting = 1u << 21;

__global__ __launch_bounds__(64) void pibt_plan_kernel(const uint8_t *__restrict__ grids, int n_grids, int n_agents, int H, int W,
                                                       const uint16_t *__restrict__ dist, const int16_t *__restrict__ pos,
                                                       const uint8_t *__restrict__ done, const uint32_t *__restrict__ since,
                                                       uint16_t *occ, int32_t *__restrict__ actions, int16_t *__restrict__ planned,
                                                       int8_t *__restrict__ log, int32_t *__restrict__ len, int max_steps, uint64_t seed,
                                                       uint64_t t, int64_t inst_offset)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint2 *stack = reinterpret_cast<uint2 *>(smem);                       // [n_agents] frames; the since values while ranking
    uint32_t *snc = reinterpret_cast<uint32_t *>(smem);
    int *cell = reinterpret_cast<int *>(stack + n_agents);                // [n_agents] current cell id
    int *nxt = cell + n_agents;                                           // [n_agents] -1 undecided, else (action << 24) | next cell id
    uint16_t *order = reinterpret_cast<uint16_t *>(nxt + n_agents);       // [n_agents] agent ids by priority

    const int inst = blockIdx.x, lane = threadIdx.x;
    const int cells = H * W;
    const size_t g0 = (size_t)inst * n_agents;
    if (done[inst] != 0) {                                                // wave-uniform: a finished instance is not planned
        for (int a = lane; a < n_agents; a += 64) {
            actions[g0 + a] = 0;
            planned[2 * (g0 + a)] = pos[2 * (g0 + a)];
            planned[2 * (g0 + a) + 1] = pos[2 * (g0 + a) + 1];
        }
        return;
    }
    const uint8_t *grid = grids + (size_t)(inst % n_grids) * cells;
    uint16_t *occ_now = occ + (size_t)inst * 2 * cells, *next_occ = occ_now + cells;

    for (int a = lane; a < n_agents; a += 64) {
        int c = (int)pos[2 * (g0 + a)] * W + (int)pos[2 * (g0 + a) + 1];
        c = min(max(c, 0), cells - 1);                                    // (env states are inside the frame)
        cell[a] = c;
        nxt[a] = -1;
        snc[a] = since[g0 + a];
        occ_now[c] = (uint16_t)a;
    }
    __syncthreads();
    for (int a = lane; a < n_agents; a += 64) {                           // rank by counting: (since desc, id asc)
        const uint32_t s = snc[a];
        int rank = 0;
        for (int b = 0; b < n_agents; b++) {
            const uint32_t sb = snc[b];
            rank += (sb > s || (sb == s && b < a)) ? 1 : 0;
        }
        order[rank] = (uint16_t)a;
    }
    __syncthreads();                                                      // order[] complete; snc[] is dead, the stack takes its place

    // ---- the serial part: every lane runs it identically (uniform branches, identical addresses and values) ----
    int sp = 0;
    bool ret = false;
    for (int oi = 0; oi < n_agents; oi++) {
        const int top = order[oi];
        if (nxt[top] >= 0) continue;
        int push_a = top, push_par = (int)kNil;
        for (;;) {
            if (push_a >= 0) {                                            // enter PIBT(push_a, push_par): form and sort its candidates
                const int a = push_a, ca = cell[a];
                const int r = ca / W, c = ca - r * W;
                const uint64_t z = splitmix_z(seed, t, (uint64_t)((inst_offset + inst) * (int64_t)n_agents + a));
                unsigned key = 0xFFFFFFF8u | (unsigned)min(lane, 7);      // dropped candidates sort last (and stay distinct)
                bool valid = false;
                if (lane < 5) {
                    const int dr = (lane == 1) ? -1 : (lane == 2 ? 1 : 0), dc = (lane == 3) ? -1 : (lane == 4 ? 1 : 0);
                    const int rr = r + dr, cc = c + dc;
                    if (rr >= 0 && rr < H && cc >= 0 && cc < W) {
                        const int u = rr * W + cc;
                        const unsigned d = dist[(g0 + a) * (size_t)cells + u];
                        if (grid[u] == 0 && d != kUnreach) {
                            const unsigned who = occ_now[u];
                            const unsigned o = (who != kNil && who != (unsigned)a) ? 1u : 0u;
                            const unsigned rk = (unsigned)(z >> (5 * lane)) & 31u;
                            key = (((d * 2u + o) * 32u + rk) * 8u) + (unsigned)lane;
                            valid = true;
                        }
                    }
                }
                int rank = 0;
#pragma unroll
                for (int j = 0; j < 5; j++) rank += (__shfl(key, j, 64) < key) ? 1 : 0;
                const unsigned contrib = valid ? ((unsigned)lane << (3 * rank)) : 0u;
                unsigned packed = 0;
#pragma unroll
                for (int j = 0; j < 5; j++) packed |= __shfl(contrib, j, 64);
                const unsigned ncand = (unsigned)__popcll(__ballot(valid));
                if (sp >= n_agents) break;                                // (cannot happen: an agent enters at most once per step)
                stack[sp] = make_uint2((unsigned)a | ((unsigned)push_par << 16), packed | (ncand << 15));
                sp++;
                push_a = -1;
            }
            if (sp == 0) break;
            const uint2 f = stack[sp - 1];
            const int a = (int)(f.x & 0xFFFFu);
            const unsigned par = f.x >> 16;
            unsigned y = f.y;
            if (y & kFrameWaiting) {                                      // back from PIBT(c, a)
                y &= ~kFrameWaiting;
                if (ret) { sp--; continue; }                              // the child found a cell: a keeps its reservation (ret stays true)
            }
            const unsigned ncand = (y >> 15) & 7u;
            unsigned idx = (y >> 18) & 7u;
            const int ca = cell[a];
            const int par_cell = (par != kNil) ? cell[par] : -1;
            bool settled = false;
            while (idx < ncand) {
                const int k = (int)((y >> (3 * idx)) & 7u);
                idx++;
                const int u = ca + ((k == 1) ? -W : (k == 2) ? W : (k == 3) ? -1 : (k == 4) ? 1 : 0);   // in the frame: checked at entry
                if (next_occ[u] != kNil) continue;                        // 1. reserved for the next step
                if (u == par_cell) continue;                              // 2. the parent's cell
                unsigned c = occ_now[u];
                if (c >= (unsigned)n_agents) c = kNil;
                const int nc = (c != kNil) ? nxt[c] : -1;
                if (nc >= 0 && (nc & 0xFFFFFF) == ca) continue;           // 3. a swap with a decided agent
                nxt[a] = (k << 24) | u;                                   // 4. reserve
                next_occ[u] = (uint16_t)a;
                settled = true;
                if (c != kNil && c != (unsigned)a && nc < 0) {            // 5. inherit the priority: PIBT(c, a)
                    stack[sp - 1].y = (y & ~(7u << 18)) | (idx << 18) | kFrameWaiting;
                    push_a = (int)c;
                    push_par = a;
                } else {
                    ret = true;                                           // 6.
                    sp--;
                }
                break;
            }
            if (!settled) {                                               // no candidate left: stay, taking the cell back from the parent
                nxt[a] = ca;
                next_occ[ca] = (uint16_t)a;
                ret = false;
                sp--;
            }
        }
    }
    __syncthreads();

    const int tl = len[inst];
    for (int a = lane; a < n_agents; a += 64) {
        const int v = nxt[a], u = v & 0xFFFFFF, k = (v >> 24) & 7;
        const int ur = u / W;
        actions[g0 + a] = k;
        planned[2 * (g0 + a)] = (int16_t)ur;
        planned[2 * (g0 + a) + 1] = (int16_t)(u - ur * W);
        if (tl < max_steps) log[(g0 + a) * (size_t)max_steps + tl] = (int8_t)k;
        occ_now[cell[a]] = (uint16_t)kNil;                                // leave the workspace all-NIL for the next step
        next_occ[u] = (uint16_t)kNil;
    }
    if (lane == 0 && tl < max_steps) len[inst] = tl + 1;
}

// after the env has stepped: since = 0 on the goal, else since + 1 (instances that are done are never planned again)
__global__ void pibt_since_kernel(const int16_t *__restrict__ pos, const int16_t *__restrict__ goal, const uint8_t *__restrict__ done,
                                  uint32_t *__restrict__ since, int n_inst, int n_agents)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_inst * n_agents) return;
    if (done[i / n_agents] != 0) return;
    const bool on = pos[2 * i] == goal[2 * i] && pos[2 * i + 1] == goal[2 * i + 1];
    since[i] = on ? 0u : since[i] + 1u;
}

}  // namespace

struct mgpt_expert {
    mgpt_tokenizer *tok = nullptr;
    mgpt_env *env = nullptr;
    int n_inst = 0, n_agents = 0, H = 0, W = 0, n_grids = 0, max_steps = 0;
    const uint8_t *grids = nullptr;             // borrowed from the tokenizer
    const uint16_t *dist = nullptr;
    const int16_t *pos = nullptr, *goal = nullptr;   // borrowed from the env
    const uint8_t *done = nullptr;
    uint64_t seed = 0, t = 0;
    int64_t inst_offset = 0;
    uint16_t *occ = nullptr;                    // [n_inst][2][H*W] occ_now | next_occ, all NIL between steps
    uint32_t *since = nullptr;                  // [n_inst][n_agents]
    int16_t *planned = nullptr;                 // [n_inst][n_agents][2]
    int8_t *log = nullptr;                      // [n_inst][n_agents][max_steps]
    int32_t *len = nullptr;                     // [n_inst]
    bool have_reset = false;
};

static size_t expert_lds_bytes(int n_agents) { return (size_t)n_agents * (sizeof(uint2) + 2 * sizeof(int) + sizeof(uint16_t)); }

// what the planner does not model: lifelong goal queues and the non-default collision rules
static int expert_check_env(const mgpt_expert *ex)
{
    int H = 0, W = 0, n_grids = 0, rules = 0, lifelong = 0;
    env_config(ex->env, &H, &W, &n_grids, &rules, &lifelong);
    MGPT_REQUIRE(!lifelong, MGPT_ERR_UNSUPPORTED, "the PIBT expert does not plan lifelong (on_target = restart) episodes");
    MGPT_REQUIRE(rules == 0, MGPT_ERR_UNSUPPORTED, "the PIBT expert plans for the default collision rules only (env rule mask %d)", rules);
    return MGPT_OK;
}

extern "C" int mgpt_expert_create(mgpt_expert **out, mgpt_tokenizer *tok, mgpt_env *env, uint64_t seed, int64_t inst_offset, int max_steps)
{
    MGPT_REQUIRE(out && tok && env, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(max_steps > 0 && inst_offset >= 0, MGPT_ERR_ARG, "bad max_steps / inst_offset");
    TokView tv;
    tok_view(tok, &tv);
    int n_inst = 0, n_agents = 0, H = 0, W = 0, n_grids = 0, rules = 0, lifelong = 0;
    env_shape(env, &n_inst, &n_agents);
    env_config(env, &H, &W, &n_grids, &rules, &lifelong);
    MGPT_REQUIRE(n_agents <= 65534, MGPT_ERR_UNSUPPORTED, "n_agents=%d: agent ids are 16 bits with 0xFFFF reserved", n_agents);
    MGPT_REQUIRE(tv.n_inst == n_inst && tv.n_agents == n_agents && tv.H == H && tv.W == W && tv.n_grids == n_grids, MGPT_ERR_ARG,
                 "tokenizer (%d x %d agents, %d x %d, %d grids) and env (%d x %d agents, %d x %d, %d grids) differ in shape", tv.n_inst,
                 tv.n_agents, tv.H, tv.W, tv.n_grids, n_inst, n_agents, H, W, n_grids);
    MGPT_REQUIRE((int64_t)H * W < (1 << 24), MGPT_ERR_UNSUPPORTED, "H*W=%lld cells: a planned cell is kept in 24 bits", (long long)H * W);
    MGPT_REQUIRE(expert_lds_bytes(n_agents) <= 64 * 1024, MGPT_ERR_UNSUPPORTED, "n_agents=%d: the stack does not fit 64 KB of LDS", n_agents);
    mgpt_expert *ex = new mgpt_expert();
    ex->tok = tok; ex->env = env; ex->n_inst = n_inst; ex->n_agents = n_agents; ex->H = H; ex->W = W; ex->n_grids = n_grids;
    ex->max_steps = max_steps; ex->seed = seed; ex->inst_offset = inst_offset;
    ex->grids = tv.grids; ex->dist = tv.dist;
    int rc = expert_check_env(ex);
    if (rc == MGPT_OK) rc = mgpt_env_state(env, &ex->pos, &ex->goal, &ex->done);
    if (rc != MGPT_OK) { delete ex; return rc; }
    const size_t total = (size_t)n_inst * n_agents;
    hipError_t e = hipMalloc(&ex->occ, (size_t)n_inst * 2 * H * W * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(&ex->since, total * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&ex->planned, total * 2 * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc(&ex->log, total * (size_t)max_steps);
    if (e == hipSuccess) e = hipMalloc(&ex->len, (size_t)n_inst * sizeof(int32_t));
    if (e != hipSuccess) {
        set_error("hipMalloc failed in mgpt_expert_create: %s", hipGetErrorString(e));
        mgpt_expert_destroy(ex);
        return MGPT_ERR_HIP;
    }
    *out = ex;
    return MGPT_OK;
}

extern "C" int mgpt_expert_destroy(mgpt_expert *ex)
{
    if (!ex) return MGPT_OK;
    (void)hipFree(ex->occ); (void)hipFree(ex->since); (void)hipFree(ex->planned); (void)hipFree(ex->log); (void)hipFree(ex->len);
    delete ex;
    return MGPT_OK;
}

extern "C" int mgpt_expert_reset(mgpt_expert *ex, void *stream)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    TokView tv;
    tok_view(ex->tok, &tv);
    MGPT_REQUIRE(tv.have_agents, MGPT_ERR_STATE, "mgpt_tokenizer_create_agents must precede mgpt_expert_reset (the planner reads its distance fields)");
    const int rc = expert_check_env(ex);
    if (rc != MGPT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)ex->n_inst * ex->n_agents;
    // occupancy is rebuilt from the env's positions by every plan launch and scattered back to NIL at its end: all-NIL is the state between steps
    MGPT_HIP(hipMemsetAsync(ex->occ, 0xFF, (size_t)ex->n_inst * 2 * ex->H * ex->W * sizeof(uint16_t), s));
    MGPT_HIP(hipMemsetAsync(ex->since, 0, total * sizeof(uint32_t), s));
    MGPT_HIP(hipMemsetAsync(ex->planned, 0, total * 2 * sizeof(int16_t), s));
    MGPT_HIP(hipMemsetAsync(ex->log, 0, total * (size_t)ex->max_steps, s));
    MGPT_HIP(hipMemsetAsync(ex->len, 0, (size_t)ex->n_inst * sizeof(int32_t), s));
    ex->t = 0;
    ex->have_reset = true;
    return MGPT_OK;
}

extern "C" int mgpt_expert_step(mgpt_expert *ex, int32_t *d_actions, void *stream)
{
    MGPT_REQUIRE(ex && d_actions, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(ex->have_reset, MGPT_ERR_STATE, "mgpt_expert_reset must precede mgpt_expert_step");
    int rc = expert_check_env(ex);
    if (rc != MGPT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    {
        ProfScope ps(P_EXPERT_PLAN, s);
        hipLaunchKernelGGL(pibt_plan_kernel, dim3(ex->n_inst), dim3(64), expert_lds_bytes(ex->n_agents), s, ex->grids, ex->n_grids, ex->n_agents,
                           ex->H, ex->W, ex->dist, ex->pos, ex->done, ex->since, ex->occ, d_actions, ex->planned, ex->log, ex->len, ex->max_steps,
                           ex->seed, ex->t, ex->inst_offset);
        MGPT_LAUNCH_CHECK();
    }
    if ((rc = mgpt_env_step(ex->env, d_actions, s)) != MGPT_OK) return rc;
    const int total = ex->n_inst * ex->n_agents;
    hipLaunchKernelGGL(pibt_since_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, ex->pos, ex->goal, ex->done, ex->since, ex->n_inst, ex->n_agents);
    MGPT_LAUNCH_CHECK();
    ex->t++;
    return MGPT_OK;
}

extern "C" int mgpt_expert_copy_plan(mgpt_expert *ex, int16_t *d_planned_out, void *stream)
{
    MGPT_REQUIRE(ex && d_planned_out, MGPT_ERR_ARG, "NULL argument");
    MGPT_HIP(hipMemcpyAsync(d_planned_out, ex->planned, (size_t)ex->n_inst * ex->n_agents * 2 * sizeof(int16_t), hipMemcpyDeviceToDevice,
                            (hipStream_t)stream));
    return MGPT_OK;
}

extern "C" int mgpt_expert_copy_log(mgpt_expert *ex, int8_t *d_log_out, int32_t *d_len_out, void *stream)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    hipStream_t s = (hipStream_t)stream;
    if (d_log_out)
        MGPT_HIP(hipMemcpyAsync(d_log_out, ex->log, (size_t)ex->n_inst * ex->n_agents * (size_t)ex->max_steps, hipMemcpyDeviceToDevice, s));
    if (d_len_out) MGPT_HIP(hipMemcpyAsync(d_len_out, ex->len, (size_t)ex->n_inst * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return MGPT_OK;
}
