// expert.hip -- a device-resident PIBT expert (priority inheritance with backtracking): the role of run_expert() in the reference's
// dataset/generate_dataset.py:214-230 and of its logging environment (experiment_setup/create_env.py:8-33, LogActions :49-60).
//
// The reference's expert is LaCAM3 under POGEMA, neither of which is in its tree.  What is built here is the configuration generator
// of such a search, one step at a time, by this project's own spec -- a weaker teacher than LaCAM: nothing
// guarantees that all agents stand on their goals at once.  A plain depth-first LaCAM search over this generator (DESIGN.md section 21,
// lacam_search_kernel below) can run in front of the episode: an instance it solves within the step cap replays its solution.  An
// opt-in corridor swap rule is the SWAP = true instantiation of both kernels.  The generator itself is one
// device function, pibt_generate, that both kernels call.  An opt-in pass between the search and the episode
// refines a found solution by replanning one agent at a time against the others' paths (refine_*_kernel below).
// Opt-in lifelong episodes keep the plan kernel and change what follows the env step: the borrowed tokenizer
// rebuilds the fields of the agents whose goal changed and pibt_lifelong_post_kernel stands in pibt_since_kernel's place.
// An opt-in collision shield for a policy (pibt_shield_kernel) runs the same generator on the policy's action
// preferences in the place of section 20's keys: the PREF = true instantiation.  Opt-in again, the shield runs on lifelong episodes
// (DESIGN.md section 35): the plan is unchanged and the same pibt_lifelong_post_kernel follows the env step, on the same state
// (mgpt_expert::Lifelong: a context is a planner or a shield, never both).  Its step index lives on the device, since a captured
// step is replayed without the host.
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

#include <vector>

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
constexpr int kFixed = 1 << 28;                 // in nxt[]: the agent's move is set by a constraint of the search (the plan kernel never sets it)

// the arrays of one instance in dynamic LDS, [n_agents] each.  each() is the one description of the layout: lds_bytes() sums it
// and lds_carve() walks it, so the launch's byte count and the kernel's pointers cannot drift apart.
struct ExpertLds {
    uint2 *stack = nullptr;                     // PIBT frames
    int *cell = nullptr;                        // current cell id
    int *nxt = nullptr;                         // -1 undecided, else fixed | (action << 24) | next cell id
    int *goalc = nullptr;                       // search only: goal cell id
    uint32_t *snc = nullptr;                    // the since values (the plan kernel ranks them in the stack's place, before the first frame)
    uint32_t *chain = nullptr;                  // search only: the constraint chain, root end first
    uint16_t *order = nullptr;                  // agent ids by priority
    uint16_t *swp = nullptr;                    // SWAP only: the swap agent of every frame, or NIL
    uint16_t *pref = nullptr;                   // shield only: every agent's candidates in preference order (pref_word below)

    template <class F>
    __host__ __device__ constexpr void each(bool swap, bool search, bool shield, F f)
    {
        f(stack, true); f(cell, true); f(nxt, true); f(goalc, search); f(snc, search); f(chain, search); f(order, true); f(swp, swap);
        f(pref, shield);
    }
};

// per agent: 18 bytes (20 with the swap rule) for the plan kernel, 30 (32) for the search, 20 for the shield
constexpr size_t lds_bytes(int n_agents, bool swap, bool search, bool shield = false)
{
    size_t bytes = 0;
    ExpertLds().each(swap, search, shield, [&](auto *&arr, bool present) { bytes += present ? (size_t)n_agents * sizeof(*arr) : 0; });
    return bytes;
}
static_assert(lds_bytes(1, false, false) == 18 && lds_bytes(1, true, false) == 20 && lds_bytes(1, false, true) == 30 && lds_bytes(1, true, true) == 32);
static_assert(lds_bytes(1, false, false, true) == 20 && lds_bytes(3, false, false, true) == 60);

// An array the kernel does not have gets the address of the next one and is never used.  The plan kernel has no snc of its own: it
// ranks the since values in the stack's place, which is dead until the first frame is pushed after the rank's barrier.
__device__ __forceinline__ ExpertLds lds_carve(char *smem, int n_agents, bool swap, bool search, bool shield = false)
{
    ExpertLds L;
    L.each(swap, search, shield, [&](auto *&arr, bool present) {
        arr = reinterpret_cast<decltype(+arr)>(smem);
        if (present) smem += (size_t)n_agents * sizeof(*arr);
    });
    if (!search) L.snc = reinterpret_cast<uint32_t *>(L.stack);
    return L;
}

// ---- the corridor swap rule: an opt-in addition to the generator, the SWAP = true instantiations -------------
// cell_degree_kernel writes, once per context, the number of free 4-neighbours of every free cell (kDegBlocked on a blocked one), so
// that a step of a walk needs no neighbour-of-neighbour grid loads.  The walks are wave-uniform serial loops, capped at H * W advances;
// within a step lanes 1..4 take the four neighbours of v_puller (one deg, one occ_now and one dist load each) and a ballot gives
// (n, other).  Everything they read was written before the last barrier (occ_now) or by every lane alike (nxt): no new barrier.
constexpr unsigned kDegBlocked = 0xFFu;

__global__ __launch_bounds__(256) void cell_degree_kernel(const uint8_t *__restrict__ grids, uint8_t *__restrict__ deg, int n_grids, int H, int W)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, cells = (int64_t)H * W;
    if (i >= (int64_t)n_grids * cells) return;
    const uint8_t *grid = grids + (i / cells) * cells;
    const int v = (int)(i % cells), r = v / W, c = v - r * W;
    unsigned d = kDegBlocked;
    if (grid[v] == 0)
        d = (r > 0 && grid[v - W] == 0) + (r + 1 < H && grid[v + W] == 0) + (c > 0 && grid[v - 1] == 0) + (c + 1 < W && grid[v + 1] == 0);
    deg[i] = (uint8_t)d;
}

// what the generator and the swap rule see of one instance: its maps, the occupancy workspace and its arrays in LDS
struct GenView {
    const uint8_t *grid;                        // [H*W]
    const uint8_t *deg;                         // [H*W] SWAP only: the degree map of this instance's grid
    const uint16_t *dist;                       // [n_agents][H*W] this instance's distance fields
    uint16_t *occ_now, *next_occ;               // [H*W] each
    ExpertLds L;
    int n_agents, H, W, cells, lane;
};

// env.hip's action numbering: 0 wait, 1 up, 2 down, 3 left, 4 right
__device__ __forceinline__ int cell_step(int k, int W) { return (k == 1) ? -W : (k == 2) ? W : (k == 3) ? -1 : (k == 4) ? 1 : 0; }
__device__ __forceinline__ int step_action(int d, int W) { return (d == 0) ? 0 : (d == -W) ? 1 : (d == W) ? 2 : (d == -1) ? 3 : 4; }

// u = neighbour k of cell v (k = 0: v itself); false outside the frame.  A flag and not a sentinel value of u: the callers branch on it as
// they did on their own bounds tests, where a select cost pibt_plan_kernel<true> 1 % on 4096 instances
__device__ __forceinline__ bool neighbour(int v, int k, int H, int W, int &u)
{
    const int r = v / W, c = v - r * W;
    const int rr = r + ((k == 1) ? -1 : (k == 2 ? 1 : 0)), cc = c + ((k == 3) ? -1 : (k == 4 ? 1 : 0));
    u = rr * W + cc;
    return rr >= 0 && rr < H && cc >= 0 && cc < W;
}

// order[] = the agents by (since desc, id asc), by counting; the caller's barriers stand before and after
__device__ __forceinline__ void rank_by_since(const uint32_t *snc, uint16_t *order, int n_agents, int lane)
{
    for (int a = lane; a < n_agents; a += 64) {
        const uint32_t s = snc[a];
        int rank = 0;
        for (int b = 0; b < n_agents; b++) {
            const uint32_t sb = snc[b];
            rank += (sb > s || (sb == s && b < a)) ? 1 : 0;
        }
        order[rank] = (uint16_t)a;
    }
}

__device__ __forceinline__ unsigned swap_D(const GenView &G, unsigned a, int v) { return G.dist[(size_t)a * G.cells + v]; }

// The frame of one step of the plan and shield kernels, from the env's state (g0 = the instance's first global row): cell / nxt / snc
// in LDS, the agents scattered into occ_now, order[] ranked.  per_agent(a, c) runs once per agent in the fill loop, with its cell.
// Returns behind the second barrier: order[] is complete, snc[] is dead and the stack takes its place.
template <class F>
__device__ __forceinline__ void frame_fill(const GenView &G, const int16_t *pos, const uint32_t *since, size_t g0, F per_agent)
{
    for (int a = G.lane; a < G.n_agents; a += 64) {
        int c = (int)pos[2 * (g0 + a)] * G.W + (int)pos[2 * (g0 + a) + 1];
        c = min(max(c, 0), G.cells - 1);                                  // (env states are inside the frame)
        G.L.cell[a] = c;
        G.L.nxt[a] = -1;
        G.L.snc[a] = since[g0 + a];
        G.occ_now[c] = (uint16_t)a;
        per_agent(a, c);
    }
    __syncthreads();
    rank_by_since(G.L.snc, G.L.order, G.n_agents, G.lane);
    __syncthreads();
}

// The plan of a step back to the env's layout, behind the generator's barrier: nxt unpacked into actions and planned, the workspace
// left all-NIL for the next step.  per_agent(a, k, was) runs once per agent with its planned action and the one actions[] held on entry.
template <class F>
__device__ __forceinline__ void plan_write_back(const GenView &G, int32_t *actions, int16_t *planned, size_t g0, F per_agent)
{
    for (int a = G.lane; a < G.n_agents; a += 64) {
        const int v = G.L.nxt[a], u = v & 0xFFFFFF, k = (v >> 24) & 7;
        const int ur = u / G.W;
        const int was = actions[g0 + a];
        actions[g0 + a] = k;
        planned[2 * (g0 + a)] = (int16_t)ur;
        planned[2 * (g0 + a) + 1] = (int16_t)(u - ur * G.W);
        per_agent(a, k, was);
        G.occ_now[G.L.cell[a]] = (uint16_t)kNil;                          // leave the workspace all-NIL for the next step
        G.next_occ[u] = (uint16_t)kNil;
    }
}

// count(v_pusher, v_puller): n = the free neighbours of v_puller that are neither v_pusher nor a dead end an agent rests in; other = the
// last of them in action order
__device__ __forceinline__ int swap_count(const GenView &G, int vp, int vq, int &other)
{
    const int k = G.lane;
    bool open = false;
    int u;
    if (k >= 1 && k <= 4 && neighbour(vq, k, G.H, G.W, u)) {
        const unsigned dg = G.deg[u];
        if (dg != kDegBlocked && u != vp) {
            open = true;
            if (dg == 1u) {
                const unsigned b = G.occ_now[u];
                if (b < (unsigned)G.n_agents && swap_D(G, b, u) == 0u) open = false;
            }
        }
    }
    const unsigned m = (unsigned)(__ballot(open) & 0x1Eull);
    other = m ? vq + cell_step(31 - __clz((int)m), G.W) : vq;
    return __popc(m);
}

__device__ __forceinline__ bool swap_required(const GenView &G, unsigned pusher, unsigned puller, int vp, int vq)
{
    unsigned dp = swap_D(G, pusher, vp), dq = swap_D(G, pusher, vq);
    for (int s = 0; s < G.cells && dq < dp; s++) {
        int other;
        const int n = swap_count(G, vp, vq, other);
        if (n >= 2) return false;
        if (n <= 0) break;
        vp = vq; vq = other;
        dp = dq; dq = swap_D(G, pusher, vq);
    }
    return swap_D(G, puller, vp) < swap_D(G, puller, vq) && (dp == 0u || dq < dp);
}

__device__ __forceinline__ bool swap_possible(const GenView &G, int vp, int vq)
{
    const int origin = vp;
    for (int s = 0; s < G.cells && vq != origin; s++) {
        int other;
        const int n = swap_count(G, vp, vq, other);
        if (n >= 2) return true;
        if (n <= 0) return false;
        vp = vq; vq = other;
    }
    return false;
}

// swap_agent(a, C) on the state at the entry of PIBT(a): ca = a's cell, c0 = its best candidate; kNil = none
__device__ __forceinline__ unsigned swap_agent(const GenView &G, unsigned a, int ca, int c0)
{
    if (c0 == ca) return kNil;
    const unsigned j = G.occ_now[c0];
    if (j < (unsigned)G.n_agents && G.L.nxt[j] < 0 && swap_required(G, a, j, ca, c0) && swap_possible(G, c0, ca)) return j;
    for (int k = 1; k <= 4; k++) {
        int u;
        if (!neighbour(ca, k, G.H, G.W, u) || u == c0 || G.deg[u] == kDegBlocked) continue;
        const unsigned b = G.occ_now[u];
        if (b >= (unsigned)G.n_agents) continue;
        if (swap_required(G, b, a, ca, c0) && swap_possible(G, c0, ca)) return b;
    }
    return kNil;
}

// a frame with a swap agent keeps its candidates in reversed order
__device__ __forceinline__ unsigned swap_reversed(unsigned packed, unsigned ncand)
{
    unsigned out = 0;
    for (unsigned i = 0; i < ncand; i++) out |= ((packed >> (3u * (ncand - 1u - i))) & 7u) << (3u * i);
    return out;
}

// the pull, on the success return of a frame that took its first candidate: the swap agent j, if still undecided, follows into a's cell
__device__ __forceinline__ void swap_pull(const GenView &G, unsigned j, int ca)
{
    if (j == kNil || G.L.nxt[j] >= 0 || G.next_occ[ca] != kNil) return;
    G.L.nxt[j] = (step_action(ca - G.L.cell[j], G.W) << 24) | ca;
    G.next_occ[ca] = (uint16_t)j;
}

// ---- the shield's preference word: an agent's candidates in preference order, 3 bits each from bit 0; a slot
// beyond the last candidate holds 7, so 16 bits carry the count too (bit 15 is 0, which leaves the frame word's count field clear)
__device__ __forceinline__ unsigned pref_count(unsigned w)
{
    const unsigned used = ~w & 0x7FFFu;                                   // an action is 0..4: its slot has a clear bit, an empty slot has none
    return used ? (unsigned)(31 - __clz((int)used)) / 3u + 1u : 0u;
}

// the monotone map of an fp32 bit pattern to u32: a total order on bit patterns, no floating-point arithmetic
__device__ __forceinline__ unsigned pref_key(unsigned bits) { return (bits & 0x80000000u) ? ~bits : bits ^ 0x80000000u; }

// valid: bit k set = action k is a candidate; first: the sampler's action, tried first if it is one; the others by descending key, ties by
// ascending k
__device__ __forceinline__ unsigned pref_word(unsigned valid, int first, const unsigned (&key)[5])
{
    unsigned w = 0x7FFFu;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        if (!((valid >> k) & 1u)) continue;
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            if (j == k || !((valid >> j) & 1u)) continue;
            const bool before = j == first || (k != first && (key[j] > key[k] || (key[j] == key[k] && j < k)));
            rank += before ? 1 : 0;
        }
        w = (w & ~(7u << (3 * rank))) | ((unsigned)k << (3 * rank));
    }
    return w;
}

// ---- the generator: PIBT for every undecided agent in priority order, on the state in LDS and the occupancy workspace ----------------
// The one copy that both kernels call.  It differs between them in the step index of the candidates' random bits (`step`: the
// episode's step, or the node's depth), the global row of agent 0 (`row0`) and FIXED: the search, whose constraints have decided
// some agents with kFixed set, fails (returns false) when an agent with no candidate left finds its own cell held by such an agent.
// FIXED = false never fails.  Every lane runs this identically (uniform branches, identical addresses and values), so it needs no
// barrier; sp < n_agents is checked where a frame is pushed.  PREF = true (the collision shield): the candidate
// order of an agent does not depend on the running step, the caller has left it in L.pref[] and a frame entry is one LDS load.
template <bool SWAP, bool FIXED, bool PREF = false>
__device__ __forceinline__ bool pibt_generate(const GenView &G, uint64_t seed, uint64_t step, int64_t row0)
{
    const int n_agents = G.n_agents, W = G.W, lane = G.lane;
    uint2 *stack = G.L.stack;
    int *cell = G.L.cell, *nxt = G.L.nxt;
    uint16_t *occ_now = G.occ_now, *next_occ = G.next_occ;
    int sp = 0;
    bool ret = false;
    for (int oi = 0; oi < n_agents; oi++) {
        const int top = G.L.order[oi];
        if (nxt[top] >= 0) continue;
        int push_a = top, push_par = (int)kNil;
        for (;;) {
            if (push_a >= 0) {                                            // enter PIBT(push_a, push_par): form and sort its candidates
                const int a = push_a, ca = cell[a];
                unsigned packed = 0, ncand;
                if constexpr (PREF) {                                     // formed by the caller before the serial part
                    packed = G.L.pref[a];
                    ncand = pref_count(packed);
                } else {
                    const uint64_t z = splitmix_z(seed, step, (uint64_t)(row0 + a));
                    unsigned key = 0xFFFFFFF8u | (unsigned)min(lane, 7);  // dropped candidates sort last (and stay distinct)
                    bool valid = false;
                    int u;
                    if (lane < 5 && neighbour(ca, lane, G.H, W, u)) {
                        const unsigned d = swap_D(G, (unsigned)a, u);
                        if (G.grid[u] == 0 && d != kUnreach) {
                            const unsigned who = occ_now[u];
                            const unsigned o = (who != kNil && who != (unsigned)a) ? 1u : 0u;
                            const unsigned rk = (unsigned)(z >> (5 * lane)) & 31u;
                            key = (((d * 2u + o) * 32u + rk) * 8u) + (unsigned)lane;
                            valid = true;
                        }
                    }
                    int rank = 0;
#pragma unroll
                    for (int j = 0; j < 5; j++) rank += (__shfl(key, j, 64) < key) ? 1 : 0;
                    const unsigned contrib = valid ? ((unsigned)lane << (3 * rank)) : 0u;
#pragma unroll
                    for (int j = 0; j < 5; j++) packed |= __shfl(contrib, j, 64);
                    ncand = (unsigned)__popcll(__ballot(valid));
                }
                if (sp >= n_agents) break;                                // (cannot happen: an agent enters at most once per step)
                if constexpr (SWAP) {                                     // the swap decision, on the state at this moment
                    const unsigned j = ncand ? swap_agent(G, (unsigned)a, ca, ca + cell_step((int)(packed & 7u), W)) : kNil;
                    if (j != kNil) packed = swap_reversed(packed, ncand);
                    G.L.swp[sp] = (uint16_t)j;
                }
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
                if (ret) {                                                // the child found a cell: a keeps its reservation (ret stays true)
                    if constexpr (SWAP)
                        if (((y >> 18) & 7u) == 1u) swap_pull(G, G.L.swp[sp - 1], cell[a]);
                    sp--;
                    continue;
                }
            }
            const unsigned ncand = (y >> 15) & 7u;
            unsigned idx = (y >> 18) & 7u;
            const int ca = cell[a];
            const int par_cell = (par != kNil) ? cell[par] : -1;
            bool settled = false;
            while (idx < ncand) {
                const int k = (int)((y >> (3 * idx)) & 7u);
                idx++;
                const int u = ca + cell_step(k, W);                       // in the frame: checked at entry
                if (next_occ[u] != kNil) continue;                        // 1. reserved for the next step (by a constraint too)
                if (u == par_cell) continue;                              // 2. the parent's cell
                unsigned c = occ_now[u];
                if (c >= (unsigned)n_agents) c = kNil;
                const int nc = (c != kNil) ? nxt[c] : -1;
                if (nc >= 0 && (nc & 0xFFFFFF) == ca) continue;           // 3. a swap with a decided (or fixed) agent
                nxt[a] = (k << 24) | u;                                   // 4. reserve
                next_occ[u] = (uint16_t)a;
                settled = true;
                if (c != kNil && c != (unsigned)a && nc < 0) {            // 5. inherit the priority: PIBT(c, a)
                    stack[sp - 1].y = (y & ~(7u << 18)) | (idx << 18) | kFrameWaiting;
                    push_a = (int)c;
                    push_par = a;
                } else {
                    ret = true;                                           // 6.
                    if constexpr (SWAP)
                        if (idx == 1u) swap_pull(G, G.L.swp[sp - 1], ca);
                    sp--;
                }
                break;
            }
            if (!settled) {                                               // no candidate left: stay, taking the cell back from the parent
                if constexpr (FIXED) {
                    unsigned holder = next_occ[ca];
                    if (holder >= (unsigned)n_agents) holder = kNil;
                    if (holder != kNil && nxt[holder] >= 0 && (nxt[holder] & kFixed)) return false;   // a's cell belongs to a fixed agent
                }
                nxt[a] = ca;
                next_occ[ca] = (uint16_t)a;
                ret = false;
                sp--;
            }
        }
    }
    return true;
}

template <bool SWAP>
__global__ __launch_bounds__(64) void pibt_plan_kernel(const uint8_t *__restrict__ grids, int n_grids, int n_agents, int H, int W,
                                                       const uint16_t *__restrict__ dist, const int16_t *__restrict__ pos,
                                                       const uint8_t *__restrict__ done, const uint32_t *__restrict__ since,
                                                       uint16_t *occ, int32_t *__restrict__ actions, int16_t *__restrict__ planned,
                                                       int8_t *__restrict__ log, int32_t *__restrict__ len, int max_steps, uint64_t seed,
                                                       uint64_t t, int64_t inst_offset, const uint8_t *__restrict__ degs)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ExpertLds L = lds_carve(smem, n_agents, SWAP, false);
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
    uint16_t *occ_now = occ + (size_t)inst * 2 * cells, *next_occ = occ_now + cells;
    const size_t map0 = (size_t)(inst % n_grids) * cells;
    const GenView G{grids + map0, SWAP ? degs + map0 : nullptr, dist + g0 * (size_t)cells, occ_now, next_occ, L, n_agents, H, W, cells, lane};

    frame_fill(G, pos, since, g0, [](int, int) {});
    pibt_generate<SWAP, false>(G, seed, t, (inst_offset + inst) * (int64_t)n_agents);
    __syncthreads();

    const int tl = len[inst];
    plan_write_back(G, actions, planned, g0, [=](int a, int k, int) {     // (by value: a capture by reference costs the kernel 3 VGPRs)
        if (tl < max_steps) log[(g0 + a) * (size_t)max_steps + tl] = (int8_t)k;
    });
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

// ---- the collision shield: section 20's PIBT on the policy's preferences --------------------------------------
// One wave64 workgroup per instance, as the plan kernel.  An agent's candidate order is a function of its five logits, the sampler's
// action and the maps, none of which the running step changes, so all preference words are formed before the serial part, one agent
// per lane in the strided loop that also fills cell / nxt / snc / occ_now: the generator (PREF = true) then loads nothing from HBM for
// keys and shuffles nothing at a frame entry.  `actions` holds the sampler's actions on entry (copied to `first`) and the planned ones
// on return; overrides[inst] grows by the agents whose planned action is not the sampler's, summed by shuffles and stored by lane 0.
// *started = 1 (lane 0 of block 0) tells the host that an episode has begun, also where the launch is replayed from a graph.
// live != NULL (retire mode): block b handles instance live[b] for b < *count, with its logits at the compact rows b * n_agents ..;
// actions, pos and every other array are indexed by the global row in both modes.  An instance that is done is left untouched.
__global__ __launch_bounds__(64) void pibt_shield_kernel(const uint8_t *__restrict__ grids, int n_grids, int n_inst, int n_agents, int H, int W,
                                                         const uint16_t *__restrict__ dist, const int16_t *__restrict__ pos,
                                                         const uint8_t *__restrict__ done, const uint32_t *__restrict__ since, uint16_t *occ,
                                                         const float *__restrict__ logits, int64_t ld, const int32_t *__restrict__ live,
                                                         const int32_t *__restrict__ count, int32_t *actions, int32_t *__restrict__ first,
                                                         int16_t *__restrict__ planned, int32_t *__restrict__ overrides,
                                                         int32_t *__restrict__ started)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ExpertLds L = lds_carve(smem, n_agents, false, false, true);
    const int lane = threadIdx.x;
    int inst = blockIdx.x;
    if (inst == 0 && lane == 0) *started = 1;                             // the episode has begun: on the device, so that a graph replay says so too
    if (live != nullptr) {                                                // wave-uniform: beyond the live list, or not an instance
        if (inst >= *count) return;
        inst = live[inst];
    }
    if (inst < 0 || inst >= n_inst || done[inst] != 0) return;            // wave-uniform: a finished instance is left untouched
    const int cells = H * W;
    const size_t g0 = (size_t)inst * n_agents;
    const float *lrow = logits + (size_t)blockIdx.x * n_agents * (size_t)ld;    // (blockIdx.x == inst without a live list)
    uint16_t *occ_now = occ + (size_t)inst * 2 * cells, *next_occ = occ_now + cells;
    const size_t map0 = (size_t)(inst % n_grids) * cells;
    const GenView G{grids + map0, nullptr, dist + g0 * (size_t)cells, occ_now, next_occ, L, n_agents, H, W, cells, lane};

    frame_fill(G, pos, since, g0, [=](int a, int c) {                     // and the preference word of every agent
        const int f = actions[g0 + a];
        first[g0 + a] = f;
        unsigned key[5], valid = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            key[k] = pref_key(__float_as_uint(lrow[(size_t)a * ld + k]));
            int u;
            if (neighbour(c, k, H, W, u) && G.grid[u] == 0 && swap_D(G, (unsigned)a, u) != kUnreach) valid |= 1u << k;
        }
        L.pref[a] = (uint16_t)pref_word(valid, f, key);
    });
    pibt_generate<false, false, true>(G, 0, 0, 0);
    __syncthreads();

    int n_over = 0;
    plan_write_back(G, actions, planned, g0, [&](int, int k, int sampled) { n_over += (k != sampled) ? 1 : 0; });
    for (int off = 32; off > 0; off >>= 1) n_over += __shfl_xor(n_over, off, 64);
    if (lane == 0) overrides[inst] += n_over;
}

// ---- lifelong episodes (DESIGN.md sections 30 and 35): the post-step kernel, in pibt_since_kernel's place when ex->lifelong is on ----
// After the env has stepped an agent that arrived already holds the next goal of its queue, so "on the goal" is decided against `held`,
// the expert's own copy of the goals the agents pursued during the step: arrived = the new cell equals the held goal, which is the env's
// own test on the same values, so the count equals the env's `reached` exactly.  Then held takes the env's goals for the next step.
// One wave64 workgroup per instance, the agents in a strided loop (a cell is one 32-bit word: row | column << 16), the arrivals of the
// step summed by shuffles and written by lane 0 to arrivals[inst][k].  `live` says the instance was not done when the step began: the
// env's done flag cannot, it is already set after the episode's last step, whose arrivals still count.  Plain vector stores only.
//
// The one kernel of the planner (mgpt_expert_step) and of the shield on lifelong episodes (mgpt_expert_shield_commit, DESIGN.md
// section 35).  The shield's launches are replayed from a captured graph and never pass the host, so the slot k of the arrivals log is
// steps[inst], the number of steps this instance has made since reset: lane 0 of the instance's own wave reads it, stores the step's
// arrivals only while 0 <= k < max_steps (a graph replayed beyond the step cap writes nothing out of range) and stores k + 1.  No
// other wave touches the counter: no race, no atomics.  The launch covers every instance, guarded by `live`; it does not read retire
// mode's live list.  For the planner k is the host's step index t, as it was when the host passed t in: live[inst] is 1 at reset and
// the kernel returns early once it is 0, for good, so an instance that reaches the slot store has run this kernel in every one of the
// host's t steps since reset, and steps[inst], 0 at reset and one more per run, equals t.
__global__ __launch_bounds__(64) void pibt_lifelong_post_kernel(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ goal,
                                                                const uint8_t *__restrict__ done, uint32_t *__restrict__ since,
                                                                uint32_t *__restrict__ held, uint8_t *__restrict__ live,
                                                                int16_t *__restrict__ arrivals, int32_t *__restrict__ steps, int n_inst,
                                                                int n_agents, int max_steps)
{
    const int inst = blockIdx.x, lane = threadIdx.x;
    if (inst >= n_inst || live[inst] == 0) return;                        // wave-uniform: done before this step, nothing moved
    const size_t g0 = (size_t)inst * n_agents;
    int n = 0;
    for (int a = lane; a < n_agents; a += 64) {
        const bool on = pos[g0 + a] == held[g0 + a];
        since[g0 + a] = on ? 0u : since[g0 + a] + 1u;
        held[g0 + a] = goal[g0 + a];
        n += on ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) {
        const int k = steps[inst];
        if (k >= 0 && k < max_steps) arrivals[(size_t)inst * max_steps + k] = (int16_t)n;
        steps[inst] = k + 1;
        live[inst] = done[inst] == 0 ? 1 : 0;
    }
}

// ---- LaCAM search over the PIBT generator ---------------------------------------------------------------
// One wave64 workgroup per instance, as above: plain depth-first LaCAM whose configuration generator is the PIBT step with a chain of
// (agent, action) constraints applied first.  The node on top of `open` lives in LDS (cells, since, order, decisions with a "fixed"
// bit); the node store, `open`, the constraint pool (a node's FIFO is a linked list through it) and an open-addressing table of node
// ids live in HBM per instance.  A launch runs at most iters_per_launch iterations per instance and leaves its state in HBM.  The
// generator is pibt_generate, the function the plan kernel calls, with FIXED = true for the spec's failure exit.
enum { S_STATUS = 0, S_ITERS, S_NODES, S_CONS, S_OPEN, S_LENGTH, S_WORDS = 8 };

struct SearchArgs {
    const uint8_t *grids;
    const uint16_t *dist;
    const int16_t *pos, *goal;
    uint16_t *occ;
    int32_t *state;                             // [n_inst][S_WORDS]
    int32_t *node_q;                            // [n_inst][node_cap][n_agents] cell ids
    uint32_t *node_since;                       // [n_inst][node_cap][n_agents]
    int4 *node_meta;                            // [n_inst][node_cap] depth, parent, FIFO head, FIFO tail
    int32_t *open;                              // [n_inst][node_cap]
    int4 *cons;                                 // [n_inst][cons_cap] parent, who | k << 16, depth, next in the FIFO
    int32_t *table;                             // [n_inst][table_size] node id or -1
    int8_t *sol;                                // [n_inst][n_agents][max_steps]
    int32_t *unfinished;                        // set to 1 by every instance that needs another launch
    int n_grids, n_agents, H, W, max_steps, max_iters, iters_per_launch, node_cap, cons_cap, table_size;
    uint64_t hash_mask, seed;
    int64_t inst_offset;
    const uint8_t *deg;                         // [n_grids][H*W] the swap rule's degree map (NULL without it)
};

template <bool SWAP>
__global__ __launch_bounds__(64) void lacam_search_kernel(const SearchArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n_agents = A.n_agents, H = A.H, W = A.W;
    const ExpertLds L = lds_carve(smem, n_agents, SWAP, true);
    int *cell = L.cell, *nxt = L.nxt, *goalc = L.goalc;
    uint32_t *snc = L.snc, *chain = L.chain;
    const uint16_t *order = L.order;

    const int inst = blockIdx.x, lane = threadIdx.x;
    int32_t *st = A.state + (size_t)inst * S_WORDS;
    if (st[S_STATUS] != 0) return;                                        // wave-uniform: this instance has its outcome
    const int cells = H * W;
    const size_t g0 = (size_t)inst * n_agents;
    uint16_t *occ_now = A.occ + (size_t)inst * 2 * cells, *next_occ = occ_now + cells;
    int32_t *nq = A.node_q + (size_t)inst * A.node_cap * n_agents;
    uint32_t *ns = A.node_since + (size_t)inst * A.node_cap * n_agents;
    int4 *nm = A.node_meta + (size_t)inst * A.node_cap;
    int32_t *open = A.open + (size_t)inst * A.node_cap;
    int4 *cons = A.cons + (size_t)inst * A.cons_cap;
    int32_t *table = A.table + (size_t)inst * A.table_size;
    const int tmask = A.table_size - 1;
    const size_t map0 = (size_t)(inst % A.n_grids) * cells;
    const GenView G{A.grids + map0, SWAP ? A.deg + map0 : nullptr, A.dist + g0 * (size_t)cells, occ_now, next_occ, L, n_agents, H, W, cells, lane};

    int status = 0, iters = st[S_ITERS], nodes = st[S_NODES], ncons = st[S_CONS], open_n = st[S_OPEN], length = 0;

    // wrap-around sum over the agents: the reduction order cannot matter
    auto hash_of = [&](const int *arr) -> uint64_t {
        uint64_t h = 0;
        for (int a = lane; a < n_agents; a += 64) h += splitmix_z(0, (uint64_t)a, (uint64_t)(arr[a] & 0xFFFFFF));
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)h, off, 64), hi = __shfl_xor((uint32_t)(h >> 32), off, 64);
            h += ((uint64_t)hi << 32) | lo;
        }
        return h;
    };

    for (int a = lane; a < n_agents; a += 64) {
        const int gc = (int)A.goal[2 * (g0 + a)] * W + (int)A.goal[2 * (g0 + a) + 1];
        goalc[a] = min(max(gc, 0), cells - 1);
    }
    if (nodes == 0) {                                                     // the first launch: the start node
        for (int a = lane; a < n_agents; a += 64) {
            int c = (int)A.pos[2 * (g0 + a)] * W + (int)A.pos[2 * (g0 + a) + 1];
            c = min(max(c, 0), cells - 1);
            nxt[a] = c;
            nq[a] = c;
            ns[a] = 0u;
        }
        __syncthreads();
        const uint64_t h = hash_of(nxt);
        cons[0] = make_int4(-1, 0, 0, -1);
        nm[0] = make_int4(0, -1, 0, 0);
        table[(int)(h & A.hash_mask & (uint64_t)tmask)] = 0;
        open[0] = 0;
        nodes = 1; ncons = 1; open_n = 1;
    }
    __syncthreads();

    int cur = -1, depth = 0;
    bool at_goal = false;
    for (int it = 0; it < A.iters_per_launch; it++) {
        if (open_n == 0) { status = 2; break; }
        if (iters >= A.max_iters) { status = 3; break; }
        iters++;
        const int top = open[open_n - 1];
        if (top != cur) {                                                 // bring the node into LDS, its occupancy into the workspace
            if (cur >= 0)
                for (int a = lane; a < n_agents; a += 64) occ_now[cell[a]] = (uint16_t)kNil;
            __syncthreads();
            bool off = false;
            for (int a = lane; a < n_agents; a += 64) {
                const int c = nq[(size_t)top * n_agents + a];
                cell[a] = c;
                snc[a] = ns[(size_t)top * n_agents + a];
                occ_now[c] = (uint16_t)a;
                off |= c != goalc[a];
            }
            at_goal = __ballot(off) == 0ull;
            __syncthreads();
            rank_by_since(snc, L.order, n_agents, lane);
            __syncthreads();
            cur = top;
            depth = nm[top].x;
        }
        if (at_goal) {                                                    // 1. solved: the solution is the parent chain
            status = depth <= A.max_steps ? 1 : 4;
            length = depth;
            if (status == 1) {
                int node = top;
                for (int t = depth - 1; t >= 0; t--) {
                    const int par = nm[node].y;
                    for (int a = lane; a < n_agents; a += 64) {
                        const int d = nq[(size_t)node * n_agents + a] - nq[(size_t)par * n_agents + a];
                        A.sol[(g0 + a) * (size_t)A.max_steps + t] = (int8_t)step_action(d, W);
                    }
                    node = par;
                }
            }
            break;
        }
        const int4 meta = nm[top];
        if (meta.z < 0) { open_n--; continue; }                           // 2. nothing left to try below this node
        const int C = meta.z;                                             // 3. the front of the FIFO, and its successors behind the tail
        const int4 ce = cons[C];
        const int cd = ce.z;
        int head = ce.w, tail = (ce.w < 0) ? -1 : meta.w;
        if (cd < n_agents) {
            const int i = order[cd];
            int u;
            const bool valid = lane < 5 && neighbour(cell[i], lane, H, W, u) && G.grid[u] == 0 && swap_D(G, (unsigned)i, u) != kUnreach;
            const unsigned mask = (unsigned)(__ballot(valid) & 31ull);
            for (int k = 0; k < 5; k++) {
                if (!((mask >> k) & 1u) || ncons >= A.cons_cap) continue; // (the pool holds one root per node and five entries per iteration)
                cons[ncons] = make_int4(C, i | (k << 16), cd + 1, -1);
                if (tail >= 0) cons[tail].w = ncons; else head = ncons;
                tail = ncons;
                ncons++;
            }
        }
        nm[top] = make_int4(meta.x, meta.y, head, tail);

        // 4. the generator: constraints first, then PIBT for the undecided agents
        for (int a = lane; a < n_agents; a += 64) nxt[a] = -1;
        __syncthreads();
        bool fail = false;
        for (int j = cd - 1, c = C; j >= 0; j--) {
            const int4 e = cons[c];
            chain[j] = (uint32_t)e.y;
            c = e.x;
        }
        for (int j = 0; j < cd; j++) {
            const int who = (int)(chain[j] & 0xFFFFu), k = (int)(chain[j] >> 16);
            const int ca = cell[who];
            const int u = ca + cell_step(k, W);                           // in the frame: checked when the constraint was made
            if (next_occ[u] != kNil) { fail = true; break; }
            unsigned c = occ_now[u];
            if (c >= (unsigned)n_agents) c = kNil;
            if (c != kNil && c != (unsigned)who) {
                const int nc = nxt[c];
                if (nc >= 0 && (nc & 0xFFFFFF) == ca) { fail = true; break; }
            }
            nxt[who] = kFixed | (k << 24) | u;
            next_occ[u] = (uint16_t)who;
        }
        if (!fail) fail = !pibt_generate<SWAP, true>(G, A.seed, (uint64_t)depth, (A.inst_offset + inst) * (int64_t)n_agents);
        __syncthreads();
        for (int a = lane; a < n_agents; a += 64) {                       // the reservations of this call go back to NIL, whatever its outcome
            const int v = nxt[a];
            if (v >= 0) next_occ[v & 0xFFFFFF] = (uint16_t)kNil;
        }
        __syncthreads();
        if (fail) continue;

        // 5. explored?  Equality of the whole configuration decides; the hash only says where to start looking
        const uint64_t h = hash_of(nxt);
        int slot = (int)(h & A.hash_mask & (uint64_t)tmask);
        bool found = false;
        for (int probe = 0; probe < A.table_size; probe++) {
            const int id = table[slot];
            if (id < 0) break;
            bool diff = false;
            for (int a = lane; a < n_agents; a += 64) diff |= nq[(size_t)id * n_agents + a] != (nxt[a] & 0xFFFFFF);
            if (__ballot(diff) == 0ull) { found = true; break; }
            slot = (slot + 1) & tmask;
        }
        if (found || nodes >= A.node_cap || ncons >= A.cons_cap || table[slot] >= 0) continue;   // (the caps cannot be reached: see mgpt_expert_set_search)

        // 6. the new node
        const int id = nodes++;
        for (int a = lane; a < n_agents; a += 64) {
            const int u = nxt[a] & 0xFFFFFF;
            nq[(size_t)id * n_agents + a] = u;
            ns[(size_t)id * n_agents + a] = (u == goalc[a]) ? 0u : snc[a] + 1u;
        }
        cons[ncons] = make_int4(-1, 0, 0, -1);
        nm[id] = make_int4(depth + 1, top, ncons, ncons);
        ncons++;
        table[slot] = id;
        open[open_n++] = id;
    }
    __syncthreads();
    if (cur >= 0)
        for (int a = lane; a < n_agents; a += 64) occ_now[cell[a]] = (uint16_t)kNil;   // leave the workspace all-NIL
    st[S_STATUS] = status; st[S_ITERS] = iters; st[S_NODES] = nodes; st[S_CONS] = ncons; st[S_OPEN] = open_n; st[S_LENGTH] = length;
    if (status == 0 && lane == 0) *A.unfinished = 1;
}

// search mode: an instance whose solution is replayed is hidden from the plan kernel (as if done) ...
__global__ void search_skip_kernel(const uint8_t *__restrict__ done, const int32_t *__restrict__ state, uint8_t *__restrict__ skip, int n_inst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_inst) skip[i] = (done[i] != 0 || state[(size_t)i * S_WORDS + S_STATUS] == 1) ? 1 : 0;
}

// ... and takes its actions, planned cells and log entry from the solution
__global__ __launch_bounds__(64) void search_replay_kernel(const int32_t *__restrict__ state, const int8_t *__restrict__ sol,
                                                           const int16_t *__restrict__ pos, const uint8_t *__restrict__ done, int n_agents,
                                                           int32_t *__restrict__ actions, int16_t *__restrict__ planned, int8_t *__restrict__ log,
                                                           int32_t *__restrict__ len, int max_steps)
{
    const int inst = blockIdx.x, lane = threadIdx.x;
    if (done[inst] != 0 || state[(size_t)inst * S_WORDS + S_STATUS] != 1) return;
    const int tl = len[inst], length = state[(size_t)inst * S_WORDS + S_LENGTH];
    const size_t g0 = (size_t)inst * n_agents;
    __syncthreads();
    for (int a = lane; a < n_agents; a += 64) {
        const int k = (tl < length && tl < max_steps) ? (int)sol[(g0 + a) * (size_t)max_steps + tl] : 0;
        actions[g0 + a] = k;
        planned[2 * (g0 + a)] = (int16_t)(pos[2 * (g0 + a)] + ((k == 1) ? -1 : (k == 2) ? 1 : 0));
        planned[2 * (g0 + a) + 1] = (int16_t)(pos[2 * (g0 + a) + 1] + ((k == 3) ? -1 : (k == 4) ? 1 : 0));
        if (tl < max_steps) log[(g0 + a) * (size_t)max_steps + tl] = (int8_t)k;
    }
    if (lane == 0 && tl < max_steps) len[inst] = tl + 1;
}

// ---- refinement of a found solution: single-agent space-time replanning ---------------------------------------
// Opt-in, between the search and the episode.  refine_path_kernel turns the parent chain of a status 1 / 4 instance whose length is
// within the horizon into a path buffer [t][agent] of cell ids with every agent's arrival time; refine_round_kernel runs one round
// (every agent with a non-zero arrival replanned once against the others' fixed paths) and is launched until no instance adopted
// anything; refine_final_kernel writes what the episode's kernels read (status, length, sol) and the statistics.
//
// One wave64 workgroup per instance.  A replan is a layered reachability sweep over (time, cell): reach[t] is a bitmask over the cells
// kept in 16-bit units in LDS, layers 0 .. horizon.  A lane owns whole units of the next layer: it forms the candidates of its unit
// with shifts of the current layer (the four moves and the wait), then drops the cells another agent stands on at t + 1 and the
// exchanges by looking into two LDS cell arrays (occ at t and at t + 1, scattered from the path buffer and cleared again by the same
// scatter), and stores the unit: plain stores only, no atomics.  The hold scan is a strided loop over (t, agent) with a wave reduction;
// the backtrack is serial in t, its five predecessor checks on five lanes and a ballot.  Per layer the wave goes through three
// barriers and one dependent load from the path buffer: the sweep is latency-bound, not ALU- or bandwidth-bound.
enum { R_ACTIVE = 0, R_LENGTH, R_FIRST_STATUS, R_FIRST_LENGTH, R_SOC_BEFORE, R_SOC_AFTER, R_ROUNDS, R_REPLANS, R_WORDS = 8 };

struct RefineLds {
    int *arr = nullptr, *goalc = nullptr;       // [n_agents] arrival times, goal cells
    uint16_t *reach = nullptr;                  // [horizon + 1][units] the layers
    uint16_t *occ = nullptr;                    // [2][cells] agent on a cell at t and at t + 1, NIL between replans
    uint16_t *mask = nullptr;                   // [3][units] free cells; cells not in column 0; cells not in column W - 1
};

constexpr size_t kRefineMaxLds = 160 * 1024;  // what one workgroup may hold on gfx950; up to 64 KB of it several instances share a CU
constexpr int refine_units(int64_t cells) { return (int)((cells + 15) / 16); }
constexpr size_t refine_lds_bytes(int n_agents, int64_t cells, int horizon)
{
    return (size_t)n_agents * 8 + ((size_t)(horizon + 1) * refine_units(cells) + 2 * (size_t)cells + 3 * (size_t)refine_units(cells)) * 2;
}

__device__ __forceinline__ RefineLds refine_carve(char *smem, int n_agents, int cells, int horizon)
{
    const int units = refine_units(cells);
    RefineLds L;
    L.arr = reinterpret_cast<int *>(smem);
    L.goalc = L.arr + n_agents;
    L.reach = reinterpret_cast<uint16_t *>(L.goalc + n_agents);
    L.occ = L.reach + (size_t)(horizon + 1) * units;
    L.mask = L.occ + 2 * (size_t)cells;
    return L;
}

// the 16 bits of layer R that start at bit p (any p: bits outside the layer are 0)
__device__ __forceinline__ unsigned reach_window(const uint16_t *R, int units, int p)
{
    const int q = p >> 4, s = p & 15;
    const unsigned lo = (q >= 0 && q < units) ? R[q] : 0u, hi = (q + 1 >= 0 && q + 1 < units) ? R[q + 1] : 0u;
    return ((lo | (hi << 16)) >> s) & 0xFFFFu;
}
__device__ __forceinline__ bool reach_bit(const uint16_t *R, int v) { return (R[v >> 4] >> (v & 15)) & 1u; }

struct RefineArgs {
    const uint8_t *grids;
    const int16_t *goal;
    const int32_t *state;                       // the search's [n_inst][S_WORDS]
    const int32_t *node_q, *open;
    const int4 *node_meta;
    int32_t *path;                              // [n_inst][horizon + 1][n_agents] cell ids
    int32_t *arr;                               // [n_inst][n_agents]
    int32_t *rstate;                            // [n_inst][R_WORDS]
    int32_t *adopted;                           // set to 1 by every instance that adopted a replan in this launch
    int n_grids, n_agents, H, W, max_steps, horizon, node_cap;
};

__global__ __launch_bounds__(64) void refine_path_kernel(const RefineArgs A)
{
    const int inst = blockIdx.x, lane = threadIdx.x, n_agents = A.n_agents;
    const int32_t *st = A.state + (size_t)inst * S_WORDS;
    int32_t *rs = A.rstate + (size_t)inst * R_WORDS;
    const int status = st[S_STATUS], length = st[S_LENGTH];
    const bool take = (status == 1 || status == 4) && length <= A.horizon;
    int64_t soc = 0;
    if (take) {                                                           // wave-uniform
        const int32_t *nq = A.node_q + (size_t)inst * A.node_cap * n_agents;
        const int4 *nm = A.node_meta + (size_t)inst * A.node_cap;
        int32_t *P = A.path + (size_t)inst * (A.horizon + 1) * n_agents;
        int node = A.open[(size_t)inst * A.node_cap + st[S_OPEN] - 1];
        for (int t = length; t >= 0 && node >= 0 && node < A.node_cap; t--) {
            for (int a = lane; a < n_agents; a += 64) P[(size_t)t * n_agents + a] = nq[(size_t)node * n_agents + a];
            node = nm[node].y;
        }
        __syncthreads();
        for (int a = lane; a < n_agents; a += 64) {                       // arrival: the start of the final stay on the goal
            const int g = P[(size_t)length * n_agents + a];
            int t = length;
            while (t > 0 && P[(size_t)(t - 1) * n_agents + a] == g) t--;
            A.arr[(size_t)inst * n_agents + a] = t;
            soc += t;
        }
        for (int off = 32; off > 0; off >>= 1) soc += __shfl_xor((int)soc, off, 64);
    }
    if (lane == 0) {
        rs[R_ACTIVE] = take ? 1 : 0; rs[R_LENGTH] = length; rs[R_FIRST_STATUS] = status; rs[R_FIRST_LENGTH] = length;
        rs[R_SOC_BEFORE] = (int)soc; rs[R_SOC_AFTER] = (int)soc; rs[R_ROUNDS] = 0; rs[R_REPLANS] = 0;
    }
}

__global__ __launch_bounds__(64) void refine_round_kernel(const RefineArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int inst = blockIdx.x, lane = threadIdx.x, n_agents = A.n_agents, H = A.H, W = A.W, cells = H * W;
    int32_t *rs = A.rstate + (size_t)inst * R_WORDS;
    if (rs[R_ACTIVE] == 0) return;                                        // wave-uniform: not refined, or a round of it adopted nothing
    const int units = refine_units(cells);
    const RefineLds L = refine_carve(smem, n_agents, cells, A.horizon);
    uint16_t *occ_a = L.occ, *occ_b = L.occ + cells;                      // the agents at t and at t + 1
    const uint16_t *free_m = L.mask, *notfirst_m = L.mask + units, *notlast_m = L.mask + 2 * units;
    int32_t *P = A.path + (size_t)inst * (A.horizon + 1) * n_agents;
    int32_t *garr = A.arr + (size_t)inst * n_agents;
    const uint8_t *grid = A.grids + (size_t)(inst % A.n_grids) * cells;
    const size_t g0 = (size_t)inst * n_agents;
    int length = rs[R_LENGTH], adopted = 0;

    for (int a = lane; a < n_agents; a += 64) {
        const int gc = (int)A.goal[2 * (g0 + a)] * W + (int)A.goal[2 * (g0 + a) + 1];
        L.goalc[a] = min(max(gc, 0), cells - 1);
        L.arr[a] = garr[a];
    }
    for (int v = lane; v < 2 * cells; v += 64) L.occ[v] = (uint16_t)kNil;
    for (int j = lane; j < units; j += 64) {
        unsigned fr = 0, nf = 0, nl = 0;
        for (int i = 0; i < 16; i++) {
            const int v = j * 16 + i, c = v % W;
            if (v < cells && grid[v] == 0) fr |= 1u << i;
            if (c != 0) nf |= 1u << i;
            if (c != W - 1) nl |= 1u << i;
        }
        L.mask[j] = (uint16_t)fr; L.mask[units + j] = (uint16_t)nf; L.mask[2 * units + j] = (uint16_t)nl;
    }
    __syncthreads();

    // scatter (or clear) the agents other than a of layer t
    auto scatter = [&](uint16_t *occ, int t, int a, bool set) {
        for (int b = lane; b < n_agents; b += 64)
            if (b != a) occ[P[(size_t)t * n_agents + b]] = set ? (uint16_t)b : (uint16_t)kNil;
    };

    for (int a = 0; a < n_agents; a++) {
        const int arr_a = L.arr[a];
        if (arr_a == 0) continue;
        const int ga = L.goalc[a];
        int hold = 0;                                                     // 1 + the last t at which another agent stands on a's goal
        for (int idx = lane; idx < (length + 1) * n_agents; idx += 64) {
            const int t = idx / n_agents, b = idx - t * n_agents;
            if (b != a && P[idx] == ga) hold = max(hold, t + 1);
        }
        for (int off = 32; off > 0; off >>= 1) hold = max(hold, __shfl_xor(hold, off, 64));
        if (hold >= arr_a) continue;                                      // T >= hold: nothing can be gained

        const int start = P[a];
        for (int j = lane; j < units; j += 64) L.reach[j] = (j == (start >> 4)) ? (uint16_t)(1u << (start & 15)) : (uint16_t)0;
        scatter(occ_a, 0, a, true);
        __syncthreads();
        int T = -1, t = 0;
        for (; t < arr_a; t++) {                                          // occ_a holds layer t
            const uint16_t *R = L.reach + (size_t)t * units;
            uint16_t *Rn = L.reach + (size_t)(t + 1) * units;
            if (t >= hold && reach_bit(R, ga)) { T = t; break; }
            scatter(occ_b, t + 1, a, true);
            __syncthreads();
            for (int j = lane; j < units; j += 64) {
                const int base = j * 16;
                unsigned m = (R[j] | (reach_window(R, units, base - 1) & notfirst_m[j]) | (reach_window(R, units, base + 1) & notlast_m[j]) |
                              reach_window(R, units, base - W) | reach_window(R, units, base + W)) & free_m[j];
                unsigned out = 0;
                while (m) {
                    const int i = __ffs((int)m) - 1, v = base + i;
                    m &= m - 1u;
                    if (occ_b[v] != kNil) continue;                       // another agent stands there at t + 1
                    const unsigned b = occ_a[v];
                    if (b != kNil) {                                      // b leaves v: a predecessor that b moves onto would be an exchange
                        bool ok = false;
                        for (int k = 0; k < 5; k++) {
                            int u;
                            ok |= neighbour(v, k, H, W, u) && reach_bit(R, u) && occ_b[u] != b;
                        }
                        if (!ok) continue;
                    }
                    out |= 1u << i;
                }
                Rn[j] = (uint16_t)out;
            }
            __syncthreads();
            scatter(occ_a, t, a, false);
            __syncthreads();
            uint16_t *tmp = occ_a; occ_a = occ_b; occ_b = tmp;
        }
        scatter(occ_a, t, a, false);                                      // t = T, or arr_a: the layer occ_a still holds
        __syncthreads();
        if (T < 0) continue;

        // adopt: backtrack from (T, ga), the first of wait, up, down, left, right whose predecessor is reached and is no exchange
        int v = ga;
        for (int tt = T; tt >= 1; tt--) {
            const uint16_t *R = L.reach + (size_t)(tt - 1) * units;
            int ex = -1;                                                  // where the agent that stands on v at tt - 1 goes
            for (int b = lane; b < n_agents; b += 64)
                if (b != a && P[(size_t)(tt - 1) * n_agents + b] == v) ex = P[(size_t)tt * n_agents + b];
            for (int off = 32; off > 0; off >>= 1) ex = max(ex, __shfl_xor(ex, off, 64));
            int u = v;
            const int back = (lane == 1) ? 2 : (lane == 2) ? 1 : (lane == 3) ? 4 : (lane == 4) ? 3 : 0;      // u = v - move[lane]
            const bool ok = lane < 5 && neighbour(v, back, H, W, u) && reach_bit(R, u) && u != ex;
            const unsigned m = (unsigned)(__ballot(ok) & 31ull);
            if (m == 0u) break;                                           // (cannot happen: v was reached from some cell of the layer before)
            if (lane == 0) P[(size_t)tt * n_agents + a] = v;
            v = __shfl(u, __ffs((int)m) - 1, 64);
        }
        for (int tt = T + 1 + lane; tt <= length; tt += 64) P[(size_t)tt * n_agents + a] = ga;
        if (lane == 0) L.arr[a] = T;
        adopted++;
        __syncthreads();
        int len = 0;
        for (int b = lane; b < n_agents; b += 64) len = max(len, L.arr[b]);
        for (int off = 32; off > 0; off >>= 1) len = max(len, __shfl_xor(len, off, 64));
        length = len;
    }

    __syncthreads();
    int soc = 0;
    for (int b = lane; b < n_agents; b += 64) {
        garr[b] = L.arr[b];
        soc += L.arr[b];
    }
    for (int off = 32; off > 0; off >>= 1) soc += __shfl_xor(soc, off, 64);
    if (lane == 0) {
        rs[R_ACTIVE] = adopted ? 1 : 0; rs[R_LENGTH] = length; rs[R_SOC_AFTER] = soc; rs[R_ROUNDS] += 1; rs[R_REPLANS] += adopted;
        if (adopted) *A.adopted = 1;
    }
}

// the final status and length into the search's state, the refined solution into sol: what search_skip_kernel / search_replay_kernel read
__global__ __launch_bounds__(64) void refine_final_kernel(const RefineArgs A, int32_t *__restrict__ state, int8_t *__restrict__ sol)
{
    const int inst = blockIdx.x, lane = threadIdx.x, n_agents = A.n_agents;
    const int32_t *rs = A.rstate + (size_t)inst * R_WORDS;
    const int first = rs[R_FIRST_STATUS];
    if ((first != 1 && first != 4) || rs[R_FIRST_LENGTH] > A.horizon) return;          // left as it is
    const int length = rs[R_LENGTH], status = length <= A.max_steps ? 1 : 4;
    const int32_t *P = A.path + (size_t)inst * (A.horizon + 1) * n_agents;
    const size_t g0 = (size_t)inst * n_agents;
    for (int idx = lane; idx < n_agents * A.max_steps; idx += 64) {
        const int a = idx / A.max_steps, t = idx - a * A.max_steps;
        int k = 0;
        if (status == 1 && t < length) k = step_action(P[(size_t)(t + 1) * n_agents + a] - P[(size_t)t * n_agents + a], A.W);
        sol[(g0 + a) * (size_t)A.max_steps + t] = (int8_t)k;
    }
    if (lane == 0) {
        state[(size_t)inst * S_WORDS + S_STATUS] = status;
        state[(size_t)inst * S_WORDS + S_LENGTH] = length;
    }
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
    // LaCAM search (mgpt_expert_set_search): all NULL / 0 without it
    bool search = false, solved = false;
    struct Search {                             // sizes and buffers, owned by search_mem
        int max_iters = 0, iters_per_launch = 0, hash_bits = 0, node_cap = 0, cons_cap = 0, table_size = 0;
        int32_t *state = nullptr, *node_q = nullptr, *open = nullptr, *table = nullptr, *unfinished = nullptr;
        uint32_t *node_since = nullptr;
        int4 *node_meta = nullptr, *cons = nullptr;
        int8_t *sol = nullptr;
        uint8_t *skip = nullptr;
    } ls;
    // the corridor swap rule (mgpt_expert_set_swap): off by default; the degree map is built when it is first turned on
    bool swap = false;
    uint8_t *deg = nullptr;                     // [n_grids][H*W]
    // refinement of found solutions (mgpt_expert_set_refine): off (max_rounds 0, all NULL) by default
    struct Refine {                             // sizes and buffers, owned by refine_mem
        int max_rounds = 0, horizon = 0;
        int32_t *path = nullptr, *arr = nullptr, *rstate = nullptr, *adopted = nullptr;
    } rf;
    // lifelong episodes: off (all NULL) by default.  One flag and one state for the planner (mgpt_expert_set_lifelong) and the shield
    // (mgpt_expert_set_shield_lifelong): which of the two it is follows from `shield`, a context is never both
    bool lifelong = false;
    struct Lifelong {                           // buffers, owned by lifelong_mem
        uint32_t *held = nullptr;               // [n_inst][n_agents] the goal every agent pursued during the step (row | column << 16)
        uint8_t *live = nullptr;                // [n_inst] the instance was not done when the last step began
        int16_t *arrivals = nullptr;            // [n_inst][max_steps] arrivals per step
        int32_t *steps = nullptr;               // [n_inst] steps made since reset: the slot of the next arrivals entry
    } lf;
    // the collision shield (mgpt_expert_set_shield): off (all NULL) by default
    bool shield = false;
    struct Shield {                             // buffers, owned by shield_mem
        int32_t *first = nullptr;               // [n_inst][n_agents] the sampler's actions of the last step
        int32_t *overrides = nullptr;           // [n_inst] agents whose planned action was not the sampler's, since reset
        int32_t *started = nullptr;             // [1] 0 at reset, 1 once a shield launch has run (a replayed graph never passes the host)
    } sh;
    DeviceArena mem, search_mem, deg_mem, refine_mem, lifelong_mem, shield_mem;   // occ .. len; ls; deg; rf; lf; sh
};

// launches the SWAP instantiation of a kernel: one wave64 workgroup per instance, its arrays in dynamic LDS
template <class... P, class... A>
static void launch_swap(const mgpt_expert *ex, bool search, void (*with)(P...), void (*without)(P...), hipStream_t s, A... args)
{
    hipLaunchKernelGGL(ex->swap ? with : without, dim3(ex->n_inst), dim3(64), lds_bytes(ex->n_agents, ex->swap, search), s, static_cast<P>(args)...);
}
constexpr int kDefaultItersPerLaunch = 512;     // the slice after which the host looks at the unfinished counter

static void refine_free(mgpt_expert *ex)
{
    ex->refine_mem.release();
    ex->rf = mgpt_expert::Refine();
}

static void search_free(mgpt_expert *ex)
{
    refine_free(ex);                                         // the pass reads the search's node store: it goes with it
    ex->search_mem.release();
    ex->ls = mgpt_expert::Search();
    ex->search = ex->solved = false;
}

// *running: an episode has begun and some instance is not done yet (reads the done flags: synchronises the device)
static int episode_running(const mgpt_expert *ex, bool *running)
{
    *running = false;
    if (!ex->have_reset) return MGPT_OK;
    if (ex->shield) {                                        // the host's t does not see the steps of a replayed graph: ask the device
        int32_t started = 0;
        MGPT_HIP(hipDeviceSynchronize());
        MGPT_HIP(hipMemcpy(&started, ex->sh.started, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (!started) return MGPT_OK;
    } else if (ex->t == 0 && !ex->solved)
        return MGPT_OK;
    std::vector<uint8_t> done((size_t)ex->n_inst);
    MGPT_HIP(hipDeviceSynchronize());
    MGPT_HIP(hipMemcpy(done.data(), ex->done, done.size(), hipMemcpyDeviceToHost));
    for (uint8_t d : done) *running |= d == 0;
    return MGPT_OK;
}

// a switch of modes (`who`: the setter's name) is refused while an episode that has begun is not over, i.e. some instance is not done
static int between_episodes(const mgpt_expert *ex, const char *who)
{
    bool running = false;
    const int rc = episode_running(ex, &running);
    if (rc != MGPT_OK) return rc;
    MGPT_REQUIRE(!running, MGPT_ERR_STATE, "%s in the middle of an episode (before mgpt_expert_reset or between episodes only)", who);
    return MGPT_OK;
}

// the lifelong state on or off, for mgpt_expert_set_lifelong and mgpt_expert_set_shield_lifelong (`who`) once their own checks have passed
static int lifelong_switch(mgpt_expert *ex, bool on, const char *who)
{
    DeviceArena mem;                                         // (off: stays empty, and the state is released by the move below)
    mgpt_expert::Lifelong lf;
    if (on) {
        const size_t ni = (size_t)ex->n_inst;
        const hipError_t e = mem.alloc_all({{&lf.held, ni * ex->n_agents * sizeof(uint32_t)}, {&lf.live, ni},
                                            {&lf.arrivals, ni * ex->max_steps * sizeof(int16_t)}, {&lf.steps, ni * sizeof(int32_t)}});
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("device allocation failed in %s (%d instances x %d agents): %s", who, ex->n_inst, ex->n_agents, hipGetErrorString(e));
            return MGPT_ERR_HIP;
        }
    }
    ex->lf = lf;
    ex->lifelong_mem = std::move(mem);
    ex->lifelong = on;
    ex->have_reset = false;                                  // on: held / live / arrivals / steps are prepared by the next reset; off: what
    return MGPT_OK;                                          // the last reset prepared was a lifelong episode's state
}

// the launch behind the env step of a lifelong episode, under the hook of the mode that asks for it
static int lifelong_post(mgpt_expert *ex, ProfId hook, hipStream_t s)
{
    ProfScope ps(hook, s);
    hipLaunchKernelGGL(pibt_lifelong_post_kernel, dim3(ex->n_inst), dim3(64), 0, s, reinterpret_cast<const uint32_t *>(ex->pos),
                       reinterpret_cast<const uint32_t *>(ex->goal), ex->done, ex->since, ex->lf.held, ex->lf.live, ex->lf.arrivals, ex->lf.steps,
                       ex->n_inst, ex->n_agents, ex->max_steps);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// copies word `words[j]` of every instance's state block ([n_inst][stride] on the device) to outs[j], [n_inst]; a NULL out is skipped
static int copy_state_words(const mgpt_expert *ex, const int32_t *state, int stride, int n, int32_t *const *outs, const int *words, hipStream_t s)
{
    for (int j = 0; j < n; j++)
        if (outs[j])
            MGPT_HIP(hipMemcpy2DAsync(outs[j], sizeof(int32_t), state + words[j], (size_t)stride * sizeof(int32_t), sizeof(int32_t), (size_t)ex->n_inst,
                                      hipMemcpyDeviceToDevice, s));
    return MGPT_OK;
}

// what the planner does not model: lifelong goal queues (unless the context's lifelong mode is on, and then the env must have them) and
// the non-default collision rules
static int expert_check_env(const mgpt_expert *ex)
{
    int H = 0, W = 0, n_grids = 0, rules = 0, lifelong = 0;
    env_config(ex->env, &H, &W, &n_grids, &rules, &lifelong);
    if (ex->lifelong && !ex->shield)
        MGPT_REQUIRE(lifelong, MGPT_ERR_STATE, "lifelong planning is on (mgpt_expert_set_lifelong): mgpt_env_set_lifelong must come first, the env has no goal queues");
    else if (ex->lifelong)
        MGPT_REQUIRE(lifelong, MGPT_ERR_STATE, "the lifelong shield is on (mgpt_expert_set_shield_lifelong): mgpt_env_set_lifelong must come first, the env has no goal queues");
    else
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
    MGPT_REQUIRE(lds_bytes(n_agents, false, false) <= 64 * 1024, MGPT_ERR_UNSUPPORTED, "n_agents=%d: the stack does not fit 64 KB of LDS", n_agents);
    mgpt_expert *ex = new mgpt_expert();
    ex->tok = tok; ex->env = env; ex->n_inst = n_inst; ex->n_agents = n_agents; ex->H = H; ex->W = W; ex->n_grids = n_grids;
    ex->max_steps = max_steps; ex->seed = seed; ex->inst_offset = inst_offset;
    ex->grids = tv.grids; ex->dist = tv.dist;
    int rc = expert_check_env(ex);
    if (rc == MGPT_OK) rc = mgpt_env_state(env, &ex->pos, &ex->goal, &ex->done);
    if (rc != MGPT_OK) { delete ex; return rc; }
    const size_t total = (size_t)n_inst * n_agents;
    const hipError_t e = ex->mem.alloc_all({{&ex->occ, (size_t)n_inst * 2 * H * W * sizeof(uint16_t)}, {&ex->since, total * sizeof(uint32_t)},
                                            {&ex->planned, total * 2 * sizeof(int16_t)}, {&ex->log, total * (size_t)max_steps},
                                            {&ex->len, (size_t)n_inst * sizeof(int32_t)}});
    if (e != hipSuccess) {
        set_error("device allocation failed in mgpt_expert_create: %s", hipGetErrorString(e));
        delete ex;
        return MGPT_ERR_HIP;
    }
    *out = ex;
    return MGPT_OK;
}

extern "C" int mgpt_expert_destroy(mgpt_expert *ex)
{
    delete ex;                                           // (its arenas free what it holds)
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
    if (ex->shield) {
        MGPT_HIP(hipMemsetAsync(ex->sh.first, 0, total * sizeof(int32_t), s));
        MGPT_HIP(hipMemsetAsync(ex->sh.overrides, 0, (size_t)ex->n_inst * sizeof(int32_t), s));
        MGPT_HIP(hipMemsetAsync(ex->sh.started, 0, sizeof(int32_t), s));
    }
    if (ex->lifelong) {                                      // held = the goals at reset; every instance is live; no arrivals and no step yet
        MGPT_HIP(hipMemcpyAsync(ex->lf.held, ex->goal, total * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        MGPT_HIP(hipMemsetAsync(ex->lf.live, 1, (size_t)ex->n_inst, s));
        MGPT_HIP(hipMemsetAsync(ex->lf.arrivals, 0, (size_t)ex->n_inst * ex->max_steps * sizeof(int16_t), s));
        MGPT_HIP(hipMemsetAsync(ex->lf.steps, 0, (size_t)ex->n_inst * sizeof(int32_t), s));
    }
    ex->t = 0;
    ex->have_reset = true;
    ex->solved = false;
    return MGPT_OK;
}

extern "C" int mgpt_expert_set_search(mgpt_expert *ex, int max_iters, int iters_per_launch, int hash_bits)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(max_iters >= 1 && max_iters <= (1 << 24), MGPT_ERR_ARG, "max_iters=%d: 1 .. 2^24", max_iters);
    MGPT_REQUIRE(iters_per_launch >= 0, MGPT_ERR_ARG, "iters_per_launch=%d: 0 (the default) or a positive count", iters_per_launch);
    MGPT_REQUIRE(hash_bits >= 0 && hash_bits <= 63, MGPT_ERR_ARG, "hash_bits=%d: 0 (the table's own size) .. 63", hash_bits);
    MGPT_REQUIRE(!ex->lifelong || ex->shield, MGPT_ERR_UNSUPPORTED,     // (a shield's lifelong mode: the shield's own refusal below)
                 "mgpt_expert_set_search with lifelong planning on (mgpt_expert_set_lifelong): the search looks for a joint goal configuration, "
                 "which a lifelong episode does not have");
    MGPT_REQUIRE(!ex->shield, MGPT_ERR_UNSUPPORTED, "mgpt_expert_set_search in shield mode (mgpt_expert_set_shield): the shield plans single steps only");
    MGPT_REQUIRE(lds_bytes(ex->n_agents, ex->swap, true) <= 64 * 1024, MGPT_ERR_UNSUPPORTED,
                 "n_agents=%d: the search's node does not fit 64 KB of LDS", ex->n_agents);
    search_free(ex);
    ex->ls.max_iters = max_iters;
    ex->ls.iters_per_launch = iters_per_launch > 0 ? iters_per_launch : kDefaultItersPerLaunch;
    ex->ls.hash_bits = hash_bits;
    ex->ls.node_cap = max_iters + 1;                            // the start node and at most one node per iteration
    ex->ls.cons_cap = ex->ls.node_cap + 5 * max_iters;             // one root per node and at most five successors per iteration
    ex->ls.table_size = 2;
    while (ex->ls.table_size < 2 * ex->ls.node_cap) ex->ls.table_size *= 2;      // load factor <= 1/2: a probe always ends on an empty slot
    const size_t ni = (size_t)ex->n_inst, na = (size_t)ex->n_agents, nc = (size_t)ex->ls.node_cap;
    const hipError_t e = ex->search_mem.alloc_all(
        {{&ex->ls.state, ni * S_WORDS * sizeof(int32_t)}, {&ex->ls.node_q, ni * nc * na * sizeof(int32_t)},
         {&ex->ls.node_since, ni * nc * na * sizeof(uint32_t)}, {&ex->ls.node_meta, ni * nc * sizeof(int4)}, {&ex->ls.open, ni * nc * sizeof(int32_t)},
         {&ex->ls.cons, ni * (size_t)ex->ls.cons_cap * sizeof(int4)}, {&ex->ls.table, ni * (size_t)ex->ls.table_size * sizeof(int32_t)},
         {&ex->ls.sol, ni * na * (size_t)ex->max_steps}, {&ex->ls.skip, ni}, {&ex->ls.unfinished, sizeof(int32_t)}});
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("device allocation failed in mgpt_expert_set_search (max_iters=%d, %d instances x %d agents): %s", max_iters, ex->n_inst, ex->n_agents,
                  hipGetErrorString(e));
        search_free(ex);
        return MGPT_ERR_HIP;
    }
    ex->search = true;
    return MGPT_OK;
}

extern "C" int mgpt_expert_set_swap(mgpt_expert *ex, int on)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(on == 0 || on == 1, MGPT_ERR_ARG, "on=%d: 0 or 1", on);
    const int rc = between_episodes(ex, "mgpt_expert_set_swap");
    if (rc != MGPT_OK) return rc;
    if (on) {
        MGPT_REQUIRE(!ex->shield, MGPT_ERR_UNSUPPORTED, "mgpt_expert_set_swap in shield mode (mgpt_expert_set_shield): the shield keeps the policy's candidate order");
        MGPT_REQUIRE(lds_bytes(ex->n_agents, true, false) <= 64 * 1024 && (!ex->search || lds_bytes(ex->n_agents, true, true) <= 64 * 1024),
                     MGPT_ERR_UNSUPPORTED, "n_agents=%d: the frames with their swap agents do not fit 64 KB of LDS", ex->n_agents);
        if (!ex->deg) {                                      // built once per context: the grids never change
            const int64_t total = (int64_t)ex->n_grids * ex->H * ex->W;
            DeviceArena mem;                                 // (ex->deg stays NULL unless the map is complete)
            uint8_t *deg = nullptr;
            MGPT_HIP(mem.alloc(&deg, (size_t)total));
            {
                ProfScope ps(P_EXPERT_CELL_DEGREE, nullptr);
                hipLaunchKernelGGL(cell_degree_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, nullptr, ex->grids, deg, ex->n_grids,
                                   ex->H, ex->W);
                MGPT_LAUNCH_CHECK();
            }
            MGPT_HIP(hipStreamSynchronize(nullptr));         // whatever stream the next step runs on finds the map complete
            ex->deg = deg;
            ex->deg_mem = std::move(mem);
        }
    }
    ex->swap = on != 0;
    return MGPT_OK;
}

extern "C" int mgpt_expert_set_lifelong(mgpt_expert *ex, int on)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(on == 0 || on == 1, MGPT_ERR_ARG, "on=%d: 0 or 1", on);
    const int rc = between_episodes(ex, "mgpt_expert_set_lifelong");
    if (rc != MGPT_OK) return rc;
    // the planner's switch: a shield's lifelong mode is not this function's to read or change, to it a shield-mode context is always off
    if (on == (ex->lifelong && !ex->shield ? 1 : 0)) return MGPT_OK;
    if (on) {
        MGPT_REQUIRE(!ex->shield, MGPT_ERR_UNSUPPORTED, "mgpt_expert_set_lifelong in shield mode (mgpt_expert_set_shield): the shield does not plan lifelong episodes");
        MGPT_REQUIRE(!ex->search, MGPT_ERR_UNSUPPORTED,
                     "mgpt_expert_set_lifelong with the search on (mgpt_expert_set_search, and mgpt_expert_set_refine with it): they look for a joint "
                     "goal configuration, which a lifelong episode does not have");
    }
    return lifelong_switch(ex, on != 0, "mgpt_expert_set_lifelong");
}

extern "C" int mgpt_expert_copy_arrivals(mgpt_expert *ex, int16_t *d_arrivals_out, void *stream)
{
    MGPT_REQUIRE(ex && d_arrivals_out, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(ex->lifelong && ex->have_reset, MGPT_ERR_STATE, "mgpt_expert_set_lifelong and mgpt_expert_reset must precede mgpt_expert_copy_arrivals");
    MGPT_HIP(hipMemcpyAsync(d_arrivals_out, ex->lf.arrivals, (size_t)ex->n_inst * ex->max_steps * sizeof(int16_t), hipMemcpyDeviceToDevice,
                            (hipStream_t)stream));
    return MGPT_OK;
}

// the refinement pass of a solve: path, rounds until none adopts anything (one device counter per launch, as the search's), final
static int refine_run(mgpt_expert *ex, hipStream_t s)
{
    RefineArgs A;
    A.grids = ex->grids; A.goal = ex->goal; A.state = ex->ls.state; A.node_q = ex->ls.node_q; A.open = ex->ls.open; A.node_meta = ex->ls.node_meta;
    A.path = ex->rf.path; A.arr = ex->rf.arr; A.rstate = ex->rf.rstate; A.adopted = ex->rf.adopted;
    A.n_grids = ex->n_grids; A.n_agents = ex->n_agents; A.H = ex->H; A.W = ex->W; A.max_steps = ex->max_steps; A.horizon = ex->rf.horizon;
    A.node_cap = ex->ls.node_cap;
    {
        ProfScope ps(P_EXPERT_REFINE_PATH, s);
        hipLaunchKernelGGL(refine_path_kernel, dim3(ex->n_inst), dim3(64), 0, s, A);
        MGPT_LAUNCH_CHECK();
    }
    const size_t lds = refine_lds_bytes(ex->n_agents, (int64_t)ex->H * ex->W, ex->rf.horizon);
    int32_t adopted = 1;
    for (int r = 0; r < ex->rf.max_rounds && adopted; r++) {
        MGPT_HIP(hipMemsetAsync(ex->rf.adopted, 0, sizeof(int32_t), s));
        {
            ProfScope ps(P_EXPERT_REFINE_ROUND, s);
            hipLaunchKernelGGL(refine_round_kernel, dim3(ex->n_inst), dim3(64), lds, s, A);
            MGPT_LAUNCH_CHECK();
        }
        MGPT_HIP(hipMemcpyAsync(&adopted, ex->rf.adopted, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        MGPT_HIP(hipStreamSynchronize(s));
    }
    {
        ProfScope ps(P_EXPERT_REFINE_FINAL, s);
        hipLaunchKernelGGL(refine_final_kernel, dim3(ex->n_inst), dim3(64), 0, s, A, ex->ls.state, ex->ls.sol);
        MGPT_LAUNCH_CHECK();
    }
    return MGPT_OK;
}

extern "C" int mgpt_expert_solve(mgpt_expert *ex, void *stream)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(!ex->shield, MGPT_ERR_STATE, "mgpt_expert_solve on a shield-mode context (mgpt_expert_set_shield): it plans through mgpt_expert_shield only");
    MGPT_REQUIRE(ex->search, MGPT_ERR_STATE, "mgpt_expert_set_search must precede mgpt_expert_solve");
    MGPT_REQUIRE(ex->have_reset && ex->t == 0, MGPT_ERR_STATE, "mgpt_expert_solve runs right after mgpt_expert_reset (the search starts from the env's positions at reset)");
    const int rc = expert_check_env(ex);
    if (rc != MGPT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t ni = (size_t)ex->n_inst;
    MGPT_HIP(hipMemsetAsync(ex->ls.state, 0, ni * S_WORDS * sizeof(int32_t), s));
    MGPT_HIP(hipMemsetAsync(ex->ls.table, 0xFF, ni * (size_t)ex->ls.table_size * sizeof(int32_t), s));
    MGPT_HIP(hipMemsetAsync(ex->ls.sol, 0, ni * (size_t)ex->n_agents * (size_t)ex->max_steps, s));
    SearchArgs A;
    A.grids = ex->grids; A.dist = ex->dist; A.pos = ex->pos; A.goal = ex->goal; A.occ = ex->occ;
    A.state = ex->ls.state; A.node_q = ex->ls.node_q; A.node_since = ex->ls.node_since; A.node_meta = ex->ls.node_meta; A.open = ex->ls.open;
    A.cons = ex->ls.cons; A.table = ex->ls.table; A.sol = ex->ls.sol; A.unfinished = ex->ls.unfinished;
    A.n_grids = ex->n_grids; A.n_agents = ex->n_agents; A.H = ex->H; A.W = ex->W; A.max_steps = ex->max_steps; A.max_iters = ex->ls.max_iters;
    A.iters_per_launch = ex->ls.iters_per_launch; A.node_cap = ex->ls.node_cap; A.cons_cap = ex->ls.cons_cap; A.table_size = ex->ls.table_size;
    A.hash_mask = ex->ls.hash_bits ? ((1ull << ex->ls.hash_bits) - 1ull) : ~0ull;
    A.seed = ex->seed; A.inst_offset = ex->inst_offset;
    A.deg = ex->swap ? ex->deg : nullptr;
    // every launch that leaves an instance unfinished has run iters_per_launch iterations of it: this many launches always suffice
    const int64_t launches = cdiv64((int64_t)ex->ls.max_iters + 1, ex->ls.iters_per_launch) + 1;
    int32_t unfinished = 1;
    for (int64_t l = 0; l < launches && unfinished; l++) {
        MGPT_HIP(hipMemsetAsync(ex->ls.unfinished, 0, sizeof(int32_t), s));
        {
            ProfScope ps(P_EXPERT_SEARCH, s);
            launch_swap(ex, true, lacam_search_kernel<true>, lacam_search_kernel<false>, s, A);
            MGPT_LAUNCH_CHECK();
        }
        MGPT_HIP(hipMemcpyAsync(&unfinished, ex->ls.unfinished, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        MGPT_HIP(hipStreamSynchronize(s));
    }
    MGPT_REQUIRE(!unfinished, MGPT_ERR_STATE, "the search left instances unfinished after %lld launches", (long long)launches);
    if (ex->rf.max_rounds > 0) {
        const int rc2 = refine_run(ex, s);
        if (rc2 != MGPT_OK) return rc2;
    }
    ex->solved = true;
    return MGPT_OK;
}

extern "C" int mgpt_expert_set_refine(mgpt_expert *ex, int max_rounds, int horizon)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(max_rounds >= 0 && max_rounds <= (1 << 16), MGPT_ERR_ARG, "max_rounds=%d: 0 (off) .. 65536", max_rounds);
    MGPT_REQUIRE(horizon == 0 || (horizon >= ex->max_steps && horizon <= (1 << 20)), MGPT_ERR_ARG,
                 "horizon=%d: 0 (twice max_steps) or max_steps=%d .. 2^20", horizon, ex->max_steps);
    MGPT_REQUIRE(ex->search, MGPT_ERR_STATE, "mgpt_expert_set_search must precede mgpt_expert_set_refine (the pass refines what the search found)");
    const int rc = between_episodes(ex, "mgpt_expert_set_refine");
    if (rc != MGPT_OK) return rc;
    if (max_rounds == 0) {
        refine_free(ex);
        return MGPT_OK;
    }
    const int hz = horizon ? horizon : 2 * ex->max_steps;
    const int64_t cells = (int64_t)ex->H * ex->W;
    const size_t lds = refine_lds_bytes(ex->n_agents, cells, hz);
    MGPT_REQUIRE(lds <= kRefineMaxLds, MGPT_ERR_UNSUPPORTED,
                 "%d x %d cells, horizon %d, %d agents: the %d reach layers of %d bytes with two cell arrays (%zu bytes in all) do not fit the "
                 "%zu bytes of LDS a workgroup may hold", ex->H, ex->W, hz, ex->n_agents, hz + 1, 2 * refine_units(cells), lds, kRefineMaxLds);
    if (lds > 64 * 1024)                                     // above the default limit of a launch's dynamic LDS
        MGPT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(refine_round_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRefineMaxLds));
    refine_free(ex);
    const size_t ni = (size_t)ex->n_inst, na = (size_t)ex->n_agents;
    const hipError_t e = ex->refine_mem.alloc_all({{&ex->rf.path, ni * (size_t)(hz + 1) * na * sizeof(int32_t)}, {&ex->rf.arr, ni * na * sizeof(int32_t)},
                                                   {&ex->rf.rstate, ni * R_WORDS * sizeof(int32_t)}, {&ex->rf.adopted, sizeof(int32_t)}});
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("device allocation failed in mgpt_expert_set_refine (horizon=%d, %d instances x %d agents): %s", hz, ex->n_inst, ex->n_agents,
                  hipGetErrorString(e));
        refine_free(ex);
        return MGPT_ERR_HIP;
    }
    ex->rf.max_rounds = max_rounds;
    ex->rf.horizon = hz;
    ex->solved = false;                                      // what a solve before this call left is not a refined result
    return MGPT_OK;
}

extern "C" int mgpt_expert_copy_refine(mgpt_expert *ex, int32_t *d_first_status, int32_t *d_first_length, int32_t *d_soc_before, int32_t *d_soc_after,
                                       int32_t *d_rounds, int32_t *d_replans, void *stream)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(ex->search && ex->solved && ex->rf.max_rounds > 0, MGPT_ERR_STATE,
                 "mgpt_expert_set_refine (max_rounds > 0) and mgpt_expert_solve must precede mgpt_expert_copy_refine");
    int32_t *outs[6] = {d_first_status, d_first_length, d_soc_before, d_soc_after, d_rounds, d_replans};
    const int words[6] = {R_FIRST_STATUS, R_FIRST_LENGTH, R_SOC_BEFORE, R_SOC_AFTER, R_ROUNDS, R_REPLANS};
    return copy_state_words(ex, ex->rf.rstate, R_WORDS, 6, outs, words, (hipStream_t)stream);
}

extern "C" int mgpt_expert_copy_search(mgpt_expert *ex, int32_t *d_status, int32_t *d_iters, int32_t *d_nodes, int32_t *d_length, void *stream)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(ex->search && ex->solved, MGPT_ERR_STATE, "mgpt_expert_solve must precede mgpt_expert_copy_search");
    int32_t *outs[4] = {d_status, d_iters, d_nodes, d_length};
    const int words[4] = {S_STATUS, S_ITERS, S_NODES, S_LENGTH};
    return copy_state_words(ex, ex->ls.state, S_WORDS, 4, outs, words, (hipStream_t)stream);
}

extern "C" int mgpt_expert_copy_solution(mgpt_expert *ex, int8_t *d_solution_out, void *stream)
{
    MGPT_REQUIRE(ex && d_solution_out, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(ex->search && ex->solved, MGPT_ERR_STATE, "mgpt_expert_solve must precede mgpt_expert_copy_solution");
    MGPT_HIP(hipMemcpyAsync(d_solution_out, ex->ls.sol, (size_t)ex->n_inst * ex->n_agents * (size_t)ex->max_steps, hipMemcpyDeviceToDevice,
                            (hipStream_t)stream));
    return MGPT_OK;
}

extern "C" int mgpt_expert_step(mgpt_expert *ex, int32_t *d_actions, void *stream)
{
    MGPT_REQUIRE(ex && d_actions, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(!ex->shield, MGPT_ERR_STATE, "mgpt_expert_step on a shield-mode context (mgpt_expert_set_shield): it plans through mgpt_expert_shield only");
    MGPT_REQUIRE(ex->have_reset, MGPT_ERR_STATE, "mgpt_expert_reset must precede mgpt_expert_step");
    int rc = expert_check_env(ex);
    if (rc != MGPT_OK) return rc;
    MGPT_REQUIRE(!ex->search || ex->solved, MGPT_ERR_STATE, "in search mode mgpt_expert_solve must precede mgpt_expert_step");
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *skip = ex->done;
    if (ex->search) {                                        // solved instances replay their solution; the plan kernel sees them as done
        hipLaunchKernelGGL(search_skip_kernel, dim3(cdiv(ex->n_inst, 256)), dim3(256), 0, s, ex->done, ex->ls.state, ex->ls.skip, ex->n_inst);
        MGPT_LAUNCH_CHECK();
        skip = ex->ls.skip;
    }
    {
        ProfScope ps(P_EXPERT_PLAN, s);
        launch_swap(ex, false, pibt_plan_kernel<true>, pibt_plan_kernel<false>, s, ex->grids, ex->n_grids, ex->n_agents, ex->H, ex->W, ex->dist, ex->pos,
                    skip, ex->since, ex->occ, d_actions, ex->planned, ex->log, ex->len, ex->max_steps, ex->seed, ex->t, ex->inst_offset,
                    ex->swap ? ex->deg : nullptr);
        MGPT_LAUNCH_CHECK();
    }
    if (ex->search) {
        hipLaunchKernelGGL(search_replay_kernel, dim3(ex->n_inst), dim3(64), 0, s, ex->ls.state, ex->ls.sol, ex->pos, ex->done, ex->n_agents, d_actions,
                           ex->planned, ex->log, ex->len, ex->max_steps);
        MGPT_LAUNCH_CHECK();
    }
    if ((rc = mgpt_env_step(ex->env, d_actions, s)) != MGPT_OK) return rc;
    if (ex->lifelong) {                                      // the fields of the agents whose goal changed, then since and the arrivals
        if ((rc = mgpt_tokenizer_update_agents(ex->tok, ex->pos, ex->goal, d_actions, 1, s)) != MGPT_OK) return rc;
        if ((rc = lifelong_post(ex, P_EXPERT_LIFELONG_POST, s)) != MGPT_OK) return rc;
        ex->t++;
        return MGPT_OK;
    }
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

// ---- the collision shield --------------------------------------------------------------------------------------
extern "C" int mgpt_expert_set_shield(mgpt_expert *ex, int on)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(on == 0 || on == 1, MGPT_ERR_ARG, "on=%d: 0 or 1", on);
    int rc = between_episodes(ex, "mgpt_expert_set_shield");
    if (rc != MGPT_OK) return rc;
    if (on == (ex->shield ? 1 : 0)) return MGPT_OK;
    if (!on) {
        (void)lifelong_switch(ex, false, "mgpt_expert_set_shield");   // (section 35's state goes with the shield; off cannot fail)
        ex->shield_mem.release();
        ex->sh = mgpt_expert::Shield();
        ex->shield = false;
        ex->have_reset = false;
        return MGPT_OK;
    }
    MGPT_REQUIRE(!ex->search && !ex->swap && ex->rf.max_rounds == 0 && !ex->lifelong, MGPT_ERR_UNSUPPORTED,
                 "mgpt_expert_set_shield together with the search, the swap rule, the refinement pass or lifelong planning: the shield runs "
                 "section 20's PIBT on the policy's candidate order, one step at a time");
    if ((rc = expert_check_env(ex)) != MGPT_OK) return rc;   // a lifelong env, a non-zero rule mask
    MGPT_REQUIRE(lds_bytes(ex->n_agents, false, false, true) <= 64 * 1024, MGPT_ERR_UNSUPPORTED,
                 "n_agents=%d: the frames with the preference words do not fit 64 KB of LDS", ex->n_agents);
    DeviceArena mem;
    mgpt_expert::Shield sh;
    const hipError_t e = mem.alloc_all({{&sh.first, (size_t)ex->n_inst * ex->n_agents * sizeof(int32_t)},
                                        {&sh.overrides, (size_t)ex->n_inst * sizeof(int32_t)}, {&sh.started, sizeof(int32_t)}});
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("device allocation failed in mgpt_expert_set_shield (%d instances x %d agents): %s", ex->n_inst, ex->n_agents, hipGetErrorString(e));
        return MGPT_ERR_HIP;
    }
    ex->sh = sh;
    ex->shield_mem = std::move(mem);
    ex->shield = true;
    ex->have_reset = false;                                  // first / overrides are prepared by the next reset
    return MGPT_OK;
}

extern "C" int mgpt_expert_shield(mgpt_expert *ex, const float *d_logits, int64_t ld, const int32_t *d_live, const int32_t *d_count,
                                  int32_t *d_actions, void *stream)
{
    MGPT_REQUIRE(ex && d_logits && d_actions, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(ld >= MGPT_NUM_ACTIONS, MGPT_ERR_ARG, "ld=%lld: a logits row holds at least %d values", (long long)ld, MGPT_NUM_ACTIONS);
    MGPT_REQUIRE((d_live == nullptr) == (d_count == nullptr), MGPT_ERR_ARG, "d_live and d_count come together (both NULL: all instances)");
    MGPT_REQUIRE(ex->shield, MGPT_ERR_STATE, "mgpt_expert_set_shield(ex, 1) must precede mgpt_expert_shield");
    MGPT_REQUIRE(ex->have_reset, MGPT_ERR_STATE, "mgpt_expert_reset must precede mgpt_expert_shield");
    const int rc = expert_check_env(ex);
    if (rc != MGPT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(P_EXPERT_SHIELD, s);
    hipLaunchKernelGGL(pibt_shield_kernel, dim3(ex->n_inst), dim3(64), lds_bytes(ex->n_agents, false, false, true), s, ex->grids, ex->n_grids,
                       ex->n_inst, ex->n_agents, ex->H, ex->W, ex->dist, ex->pos, ex->done, ex->since, ex->occ, d_logits, ld, d_live, d_count,
                       d_actions, ex->sh.first, ex->planned, ex->sh.overrides, ex->sh.started);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

extern "C" int mgpt_expert_shield_commit(mgpt_expert *ex, void *stream)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(ex->shield && ex->have_reset, MGPT_ERR_STATE, "mgpt_expert_set_shield and mgpt_expert_reset must precede mgpt_expert_shield_commit");
    if (ex->lifelong)                                        // section 35: since against the goals held during the step, and the arrivals
        return lifelong_post(ex, P_EXPERT_SHIELD_LIFELONG_POST, (hipStream_t)stream);   // (the tokenizer is not called here: the caller rebuilds the fields once per step)
    const int total = ex->n_inst * ex->n_agents;
    hipLaunchKernelGGL(pibt_since_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, ex->pos, ex->goal, ex->done, ex->since, ex->n_inst,
                       ex->n_agents);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;                                          // (no host step counter: a captured step is replayed without this call)
}

// ---- the shield on lifelong episodes ---------------------------------------------------------------------------
extern "C" int mgpt_expert_set_shield_lifelong(mgpt_expert *ex, int on)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(on == 0 || on == 1, MGPT_ERR_ARG, "on=%d: 0 or 1", on);
    MGPT_REQUIRE(ex->shield, MGPT_ERR_STATE, "mgpt_expert_set_shield(ex, 1) must precede mgpt_expert_set_shield_lifelong: it switches a shield-mode context");
    const int rc = between_episodes(ex, "mgpt_expert_set_shield_lifelong");
    if (rc != MGPT_OK) return rc;
    if (on == (ex->lifelong ? 1 : 0)) return MGPT_OK;        // (on a shield-mode context the one flag is this mode's)
    return lifelong_switch(ex, on != 0, "mgpt_expert_set_shield_lifelong");
}

extern "C" int mgpt_expert_copy_shield(mgpt_expert *ex, int32_t *d_first_out, int32_t *d_overrides_out, void *stream)
{
    MGPT_REQUIRE(ex, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(ex->shield && ex->have_reset, MGPT_ERR_STATE, "mgpt_expert_set_shield and mgpt_expert_reset must precede mgpt_expert_copy_shield");
    hipStream_t s = (hipStream_t)stream;
    if (d_first_out)
        MGPT_HIP(hipMemcpyAsync(d_first_out, ex->sh.first, (size_t)ex->n_inst * ex->n_agents * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (d_overrides_out)
        MGPT_HIP(hipMemcpyAsync(d_overrides_out, ex->sh.overrides, (size_t)ex->n_inst * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return MGPT_OK;
}

// what step.hip asks of the expert it is handed (mgpt_step_set_shield)
void mgpt::expert_contexts(const mgpt_expert *ex, const mgpt_tokenizer **tok, const mgpt_env **env, bool *shield)
{
    *tok = ex->tok; *env = ex->env; *shield = ex->shield;
}
