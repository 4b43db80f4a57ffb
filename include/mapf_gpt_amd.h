/*
 * mapf_gpt_amd.h -- C ABI of libmapf_gpt_amd.so, the MI355X (gfx950) implementation of
 * MAPF-GPT's per-step hot path:  env step -> observation tokenizer -> GPT forward -> action.
 *
 * This is the drop-in boundary.  Every entry point names the reference interface it replaces
 * (file:line in CognitiveAISystems/MAPF-GPT).  Conventions:
 *   - plain C types only; every `d_*` pointer is a DEVICE pointer (HBM) owned by the caller;
 *   - every call is stream-ordered on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and returns without synchronising unless its comment says otherwise;
 *   - returns MGPT_OK or an error code; no exception crosses the ABI; mgpt_last_error() gives a
 *     thread-local message for the last failing call;
 *   - contexts own their internal device state; the caller owns every buffer it passes in;
 *   - a context may be used from one thread at a time; different contexts are independent
 *     (no hidden globals besides the per-thread error string);
 *   - the library never falls back to the CPU: with no HIP device every compute call fails.
 *
 * Coordinates are (row, col) int16 pairs in the PADDED map frame (5 obstacle cells on every
 * side), exactly what the reference hands to its tokenizer (inference.py:130-131).
 */
#ifndef MAPF_GPT_AMD_H
#define MAPF_GPT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGPT_OK 0
#define MGPT_ERR_ARG 1          /* bad argument (NULL, size, unsupported shape)              */
#define MGPT_ERR_HIP 2          /* a HIP runtime call failed (message has hipGetErrorString) */
#define MGPT_ERR_STATE 3        /* call order violated (e.g. tokens before create_agents)    */
#define MGPT_ERR_UNSUPPORTED 4  /* shape/precision outside what the kernels implement        */

#define MGPT_CONTEXT 256        /* tokens per observation row (observation_generator.cpp:386) */
#define MGPT_VOCAB 67           /* observation_generator.cpp:321-344                          */
#define MGPT_NUM_ACTIONS 5      /* model.py:250-252                                           */

/* thread-local text of the last error on this thread ("" if none) */
const char *mgpt_last_error(void);
/* ABI version (major*1000 + minor) */
int mgpt_abi_version(void);
/* number of visible HIP devices (0 and MGPT_OK when there is none) */
int mgpt_device_count(int *count);
/* test/debug: device and pinned-host allocations this library holds at the moment, process-wide, and their bytes (either may be NULL);
 * every context's memory is counted from its allocation to its release, so a destroyed context leaves both where they were */
int mgpt_mem_debug(int64_t *live_allocs, int64_t *live_bytes);

/* ------------------------------------------------------------------------------------------
 * Tokenizer: replaces the pybind module `observation_generator`
 * (observation_generator.cpp:546-563), batched over many env instances.
 * ------------------------------------------------------------------------------------------ */

/* = struct InputParameters, observation_generator.h:22-40 / ctor args cpp:551.  All fields are honoured (kernel arguments: the
 * vocabulary -L..L -> 0..2L, -4L, -2L, +2L, six action letters, sixteen bit strings, "!" = 2L+26 of Encoder::Encoder cpp:321-350,
 * the (2 obs_radius + 1)^2 window cpp:288-311, the (2 agents_radius + 1)^2 neighbour scan and the num_agents records of
 * 5 + num_previous_actions tokens cpp:352-389, 487-512) within what the kernels' layouts hold:
 *   1 <= cost2go_value_limit <= 100, 1 <= num_agents <= 16, 0 <= num_previous_actions <= 5, 1 <= obs_radius <= 5,
 *   0 <= agents_radius <= min(5, cost2go_value_limit)   (beyond the limit the reference itself throws: int_vocab.at, cpp:358-359),
 *   (2 obs_radius + 1)^2 + num_agents (5 + num_previous_actions) <= 256 and context_size == 256: the reference pads every row to
 *   256 tokens whatever context_size says (cpp:386-387) and returns LONGER rows when they do not fit; this ABI's rows are 256 tokens.
 * Anything else -> MGPT_ERR_UNSUPPORTED.  Pinned by rows written by the compiled reference for six non-default sets
 * (tests/golden/tokp_*.npz).  The reference itself only ever passes (20, 13, 5, 256, 5, 5) (inference.py:15-29).
 * save_cost2go only steers the reference's CPU caching of distance fields (cpp:43-132) and is ignored.  grid_step (> 0,
 * and >= max(H, W) / 256) is the side of the reference's cost-to-go tiles: it changes no token except through the one
 * unseeded corner cell of an agent's cached 2*grid_step + 1 window (cpp:178-198), which is reproduced. */
typedef struct mgpt_input_parameters {
    int32_t cost2go_value_limit;
    int32_t num_agents;
    int32_t num_previous_actions;
    int32_t context_size;
    int32_t obs_radius;
    int32_t agents_radius;
    int32_t grid_step;
    int32_t save_cost2go;
} mgpt_input_parameters;

typedef struct mgpt_tokenizer mgpt_tokenizer;

/* = ObservationGenerator::ObservationGenerator(grid, cfg), observation_generator.h:112-119, for
 * n_inst instances x n_agents agents sharing one padded frame H x W.  `n_grids` distinct obstacle
 * maps are stored; instance i uses map i % n_grids (n_grids == 1: one shared map). */
int mgpt_tokenizer_create(mgpt_tokenizer **out, const mgpt_input_parameters *cfg,
                          int n_inst, int n_agents, int H, int W, int n_grids);
int mgpt_tokenizer_destroy(mgpt_tokenizer *tok);
/* = the size of Encoder's vocabulary (cpp:321-350): 2 cost2go_value_limit + 27 -- the integers -limit .. limit, the three sentinels,
 * six actions, sixteen direction strings and "!".  67 for the reference's limit of 20 = the vocab_size of every released model (model.py:110).
 * A policy whose embedding has fewer rows cannot take this tokenizer's rows: the reference's nn.Embedding raises IndexError there,
 * mgpt_step_create returns MGPT_ERR_UNSUPPORTED, and mgpt_gpt_forward does not look at the ids it is given. */
int mgpt_tokenizer_vocab_size(const mgpt_tokenizer *tok, int *out);

/* the `grid` ctor argument (h:112): d_grids = uint8 [n_grids, H, W], non-zero = blocked */
int mgpt_tokenizer_set_grids(mgpt_tokenizer *tok, const uint8_t *d_grids, void *stream);

/* = create_agents(positions, goals), cpp:391-410: history <- "n"x5, one BFS distance-to-goal field
 * per agent (cpp:200-286), greedy-direction bits (cpp:412-430).
 * d_pos, d_goal: int16 [n_inst, n_agents, 2]. */
int mgpt_tokenizer_create_agents(mgpt_tokenizer *tok, const int16_t *d_pos, const int16_t *d_goal,
                                 void *stream);

/* = update_agents(positions, goals, actions), cpp:432-485.  d_actions: int32 [n_inst, n_agents],
 * the policy's previous INTENDED actions (inference.py:140-144,168); values outside 0..4 append "n".
 * goals_may_change != 0 re-runs the BFS of every agent whose goal differs (cpp:464-468);
 * 0 skips that comparison (on_target = "nothing": goals never change). */
int mgpt_tokenizer_update_agents(mgpt_tokenizer *tok, const int16_t *d_pos, const int16_t *d_goal,
                                 const int32_t *d_actions, int goals_may_change, void *stream);
/* The same for a subset of the instances: d_active uint8 [n_inst] (NULL = all); instances with 0 keep their state (position,
 * action history, goal, distance field) untouched -- what the adapter needs when one act_batch call (inference.py:151-172)
 * presents only some of the environment slots that share a tokenizer context. */
int mgpt_tokenizer_update_agents_masked(mgpt_tokenizer *tok, const int16_t *d_pos, const int16_t *d_goal,
                                        const int32_t *d_actions, const uint8_t *d_active, int goals_may_change, void *stream);

/* = generate_observations(), cpp:516-528.  d_tokens: uint8 [n_inst * n_agents, 256], row-major,
 * row = inst * n_agents + agent.  Token ids are < 2 * cost2go_value_limit + 27 (67 by default) and fit a byte (the reference
 * widens them to int64 only for torch.nn.Embedding, inference.py:91,97).  Positions of one instance must be
 * pairwise distinct (always true for env states). */
int mgpt_tokenizer_generate_observations(mgpt_tokenizer *tok, uint8_t *d_tokens, void *stream);

/* test/debug read-backs (device pointers into the context's state, valid until destroy):
 * distance fields uint16 [n_inst, n_agents, H, W]; agent records 16 B each
 * {int16 pos_r,pos_c,goal_r,goal_c; uint8 hist[5]; uint8 next; uint8 org[2]}, org = origin (row / 64, col / 64) of the
 * partial cost-to-go window the reference would hold for the agent (observation_generator.cpp:204-207, 469-477). */
int mgpt_tokenizer_state(mgpt_tokenizer *tok, const uint16_t **d_dist, const void **d_records);
/* same state copied into caller-owned device buffers (either may be NULL) */
int mgpt_tokenizer_copy_state(mgpt_tokenizer *tok, uint16_t *d_dist_out, void *d_records_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Environment step: the part of the loop the reference delegates to POGEMA
 * (experiment_setup/create_env.py:36-46; call shape create_env.py:14-20).  POGEMA is not in the
 * reference tree: this implements the spec in DESIGN.md ("Env step spec"), parity unpinned.
 * ------------------------------------------------------------------------------------------ */
typedef struct mgpt_env mgpt_env;

int mgpt_env_create(mgpt_env **out, int n_inst, int n_agents, int H, int W, int n_grids,
                    int max_episode_steps);
int mgpt_env_destroy(mgpt_env *env);
int mgpt_env_set_grids(mgpt_env *env, const uint8_t *d_grids, void *stream);
/* = env.reset(): copies starts/goals (int16 [n_inst,n_agents,2]) and clears episode counters. */
int mgpt_env_reset(mgpt_env *env, const int16_t *d_pos, const int16_t *d_goal, void *stream);
/* = env.step(actions): d_actions int32 [n_inst, n_agents] in {0 wait,1 up,2 down,3 left,4 right}.
 * Instances that are already done ignore the actions. */
int mgpt_env_step(mgpt_env *env, const int32_t *d_actions, void *stream);
/* device views of the env state: pos/goal int16 [n_inst,n_agents,2]; done uint8 [n_inst]
 * (1 terminated = all on goal, 2 truncated = max_episode_steps reached); */
int mgpt_env_state(mgpt_env *env, const int16_t **d_pos, const int16_t **d_goal, const uint8_t **d_done);
/* the same state copied (stream-ordered, device to device) into caller-owned buffers; any may be NULL */
int mgpt_env_copy_state(mgpt_env *env, int16_t *d_pos_out, int16_t *d_goal_out, uint8_t *d_done_out, void *stream);
/* The reference-shaped list API (create_env.py:14-15: step(list) -> lists) in one call: h_actions int32 [n_inst * n_agents] on
 * the HOST (NULL: no step, just read the state back, e.g. after reset), state back into the HOST buffer
 * h_state_out = [pos int16 n*2 | goal int16 n*2 | done uint8 n_inst], n = n_inst * n_agents.  Synchronises `stream`. */
int mgpt_env_step_host(mgpt_env *env, const int32_t *h_actions, uint8_t *h_state_out, void *stream);
/* per-instance episode metrics, float32 [n_inst, 6] = {CSR, ISR, SoC, makespan, ep_length, avg_agents_density}
 * (the keys the reference's result tables use: eval_configs/05-puzzles/05-puzzles.yaml:49-58; avg_agents_density =
 * POGEMA's AgentsDensityWrapper of experiment_setup/create_env.py:38: mean over the reset observation and every step of
 * the agents' mean [agents in the 11 x 11 window / traversable cells of the window]). */
int mgpt_env_metrics(mgpt_env *env, float *d_metrics, void *stream);

/* Collision-rule switches (bit mask, default 0 = the spec of DESIGN.md section 4).  The two places where that spec rests on
 * recalled -- not verifiable offline -- POGEMA behaviour are switchable, so that pinning against fixtures captured from POGEMA
 * (tests/golden/make_golden_env.py) is a flag flip, not a rewrite:
 *   MGPT_ENV_RULE_NO_FOLLOW (1)    a move into a cell another agent occupies at the start of the step becomes wait even if
 *                                  that agent leaves it (default: following a leaving agent is allowed);
 *   MGPT_ENV_RULE_LOWEST_WINS (2)  a contested empty cell goes to the lowest-id mover (default: every claimant waits).
 * A captured step graph stays valid: the mask is a kernel argument of the next capture (the call bumps the env generation). */
#define MGPT_ENV_RULE_NO_FOLLOW 1
#define MGPT_ENV_RULE_LOWEST_WINS 2
int mgpt_env_set_rules(mgpt_env *env, int rules);

/* Lifelong mode (POGEMA on_target="restart", experiment_setup/create_env.py:28-32): d_goal_queue is int16
 * [n_inst][n_agents][queue_len][2] (padded coords); an agent that ends a step on its goal takes the next entry of its
 * queue (wrapping) and the arrival is counted; episodes then end by truncation only.  NULL / 0 switches back to
 * on_target="nothing".  Call before mgpt_env_reset.  d_reached_out: int32 [n_inst][n_agents] arrivals so far. */
int mgpt_env_set_lifelong(mgpt_env *env, const int16_t *d_goal_queue, int queue_len, void *stream);
int mgpt_env_lifelong_counts(mgpt_env *env, int32_t *d_reached_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Policy forward: replaces GPT.forward / GPT.act (mapf_gpt/model.py:167-189, 244-260).
 * ------------------------------------------------------------------------------------------ */
typedef struct mgpt_gpt mgpt_gpt;

#define MGPT_PREC_F32 0     /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32): the 1e-5 parity path        */
#define MGPT_PREC_F16X3 1   /* split-fp16 (hi/lo, 3 MFMA passes, fp32 accumulate): ~fp32 accuracy     */
#define MGPT_PREC_BF16 2    /* single-pass bf16 MFMA, fp32 accumulate: the reference's autocast mode  */

/* = GPTConfig + GPT.__init__ (model.py:107-145): vocab 67; dropout is the identity at inference (inference.py:85 net.eval()).
 * bias (model.py:115; False in every released config): a checkpoint has bias vectors iff mgpt_gpt_set_param is handed any
 * "*.bias" tensor -- see there.  max_rows = largest batch one forward call will see (activation workspace is sized for it). */
int mgpt_gpt_create(mgpt_gpt **out, int n_layer, int n_head, int n_embd, int block_size, int max_rows);
int mgpt_gpt_destroy(mgpt_gpt *gpt);

/* = load_state_dict (inference.py:83).  `name` is the reference state_dict key
 * ("transformer.h.3.attn.c_attn.weight", ...; lm_head.weight is tied to transformer.wte.weight,
 * model.py:138, either name sets both).  data: float32, HOST or DEVICE pointer (is_device),
 * n_elem must match the parameter's size.  Synchronous.
 * GPTConfig.bias = True checkpoints (model.py:14-17 LayerNorm bias; model.py:29,31,79,81 nn.Linear bias): their seven kinds of
 * "*.bias" tensors ("transformer.ln_f.bias", "transformer.h.N.{ln_1,ln_2}.bias", "...attn.c_attn.bias", "...attn.c_proj.bias",
 * "...mlp.c_fc.bias", "...mlp.c_proj.bias") are accepted; once one is set, mgpt_gpt_finalize wants all of them.  Only the
 * MGPT_PREC_F32 kernels carry bias terms: MGPT_PREC_F16X3 requests follow the envelope policy (the checkpoint counts as outside:
 * fallback = served in fp32, refuse / ignore = MGPT_ERR_UNSUPPORTED), MGPT_PREC_BF16 requests return MGPT_ERR_UNSUPPORTED. */
int mgpt_gpt_set_param(mgpt_gpt *gpt, const char *name, const float *data, int64_t n_elem, int is_device);
/* call once after all parameters are set (builds the packed operand planes of the chosen precisions) */
int mgpt_gpt_finalize(mgpt_gpt *gpt);

/* = GPT.forward(idx)[0][:, -1, :] (model.py:167-189): d_tokens uint8 [rows, 256] ->
 * d_logits float32 [rows, 67] (logits of the LAST position, the only ones the reference computes
 * at inference, model.py:186). */
int mgpt_gpt_forward(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, float *d_logits,
                     int precision, void *stream);

/* = GPT.forward(idx) for idx of T <= block_size tokens per row (model.py:167-175, "Cannot forward sequence of length t, block size is only
 * block_size" :170): d_tokens uint8 [rows, T] -> d_logits float32 [rows, 67], the logits of position T - 1.  mgpt_gpt_create accepts
 * block_size 1 .. 256 (transformer.wpe.weight is [block_size, C]); models with block_size < 256 are served by this entry point only.  Exact-fp32
 * kernels whatever the model's usual precision: the hot path (tokenizer rows, inference.py:145) is 256 tokens and never comes here. */
int mgpt_gpt_forward_t(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, int T, float *d_logits, void *stream);

/* = GPT.forward(idx, targets) (model.py:167-184): logits of EVERY position + cross-entropy terms of the targeted ones.
 * d_logits [rows][T][67] fp32 or NULL; d_targets int32 [rows][T] (-1 = ignored, model.py:183) or NULL;
 * d_row_nll [rows] fp32 = sum over the row's targeted positions of -log softmax(logits)[target], d_row_count [rows] int32
 * (both NULL iff d_targets is).  T == 256: the kernels of `precision` (resolved as by mgpt_gpt_forward); T < 256: exact fp32.
 * Targets outside [-1, 67): NaN. */
int mgpt_gpt_forward_seq(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, int T, float *d_logits, const int32_t *d_targets,
                         float *d_row_nll, int32_t *d_row_count, int precision, void *stream);

/* Scoring against one action per row (dataset gt_actions: targets -1 except position 255, fast_data_loader.py:34,58):
 * the forward of mgpt_gpt_forward (last-layer shortcut, same kernels, same logits), then d_row_nll[r] = -log softmax(logits[r])[target[r]]
 * over all 67 logits and d_row_hit[r] = (greedy action of mgpt_gpt_act(do_sample = 0) == target[r]).  d_logits [rows][67] optional.
 * Targets outside [0, 67): NaN, no hit. */
int mgpt_gpt_score_last(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, const int32_t *d_targets, float *d_row_nll,
                        int32_t *d_row_hit, float *d_logits, int precision, void *stream);

/* = GPT.act (model.py:244-260): softmax over logits[:5]; do_sample != 0 draws from it with the
 * library's counter-based RNG keyed by (seed, step, row0 + row) -- torch.multinomial's stream is
 * device-specific and not reproduced -- else arg-max.  row0 = GLOBAL id of this call's first row, so
 * that a shard of a larger job (instances split over GPUs) draws exactly what the unsharded job
 * draws for the same rows.  d_actions int32 [rows].
 * d_logits may be NULL, else float32 [rows, 67] is also written. */
int mgpt_gpt_act(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, int32_t *d_actions, float *d_logits,
                 int do_sample, uint64_t seed, uint64_t step, uint64_t row0, int precision, void *stream);

/* test/debug: copy an fp32-path workspace buffer (valid after mgpt_gpt_forward with MGPT_PREC_F32):
 * which 0 = residual stream x [rows*256, C], 1 = last LayerNorm output, 2 = q|k|v planes
 * [3][rows][n_head][256][hs], 3 = MLP hidden [rows*256, 4C]; n_elem floats from the start. */
int mgpt_gpt_debug_copy(mgpt_gpt *gpt, int which, float *d_out, int64_t n_elem, void *stream);

/* test/debug: raw bytes of a 16-bit-path workspace buffer (valid after a forward in `precision`):
 * which 0 = LayerNorm stats float2[rows*256]; 1/2 = q|k planes hi/lo; 3/4 = v^T planes hi/lo;
 * 5/6 = attention output planes hi/lo; 7/8 = MLP hidden planes hi/lo (lo only for MGPT_PREC_F16X3). */
int mgpt_gpt_debug_copy_raw(mgpt_gpt *gpt, int precision, int which, void *d_out, int64_t nbytes, void *stream);

/* Precision envelope of MGPT_PREC_F16X3 (split-fp16 MFMA passes, fp32 accumulate).  The 1e-5 logit bar of that mode is established
 * on checkpoints whose block matrices stay within max|w| <= MGPT_ENVELOPE_MAX_W and rms(w) <= MGPT_ENVELOPE_MAX_RMS (N(0, 0.02)-family
 * weights up to x4 in scale and x20 outliers on 1 % of the entries: tests/test_gpu_parity_r2.py, profiles/r0*_parity_records.jsonl);
 * beyond that (x8 scale, x100 outliers) it is 2e-5 .. 1e-3.  So the envelope is a run-time property of the loaded checkpoint:
 * mgpt_gpt_finalize measures max|w| and rms(w) of every 2-D block matrix, and the first MGPT_PREC_F16X3 forward runs
 * MGPT_ENVELOPE_PROBE_ROWS fixed pseudo-random token rows through the exact-fp32 path and through the split path in BOTH of its call
 * regimes (the kernels that serve calls of <= 128 rows and those of larger calls differ in arithmetic) and compares the logits.  The bar
 * is max(MGPT_ENVELOPE_PROBE_TOL, MGPT_ENVELOPE_PROBE_REL * max |fp32 logit|): 1e-5 absolute while the logits are of order one, where
 * the 1e-5 of the reference comparison was established; relative beyond (64 eps_f32: the fp32 forward itself moves by several
 * eps * |logit| between summation orders -- the reference's own fp32 run is 3.6e-5 from its fp64 run at |logits| ~ 4, SURVEY.md
 * appendix B).  The first such forward synchronises its stream and cannot sit inside a stream capture (MGPT_ERR_STATE).
 * A checkpoint outside either test is served according to the policy:
 *   MGPT_ENVELOPE_FALLBACK (default)  MGPT_PREC_F16X3 requests run the MGPT_PREC_F32 kernels; one line on stderr says so
 *   MGPT_ENVELOPE_REFUSE              MGPT_PREC_F16X3 requests fail with MGPT_ERR_UNSUPPORTED
 *   MGPT_ENVELOPE_IGNORE              no test, the split path runs (parity experiments)
 * Follows reference mapf_gpt/inference.py:72-85 (a loaded checkpoint is served as is, in fp32). */
#define MGPT_ENVELOPE_FALLBACK 0
#define MGPT_ENVELOPE_REFUSE 1
#define MGPT_ENVELOPE_IGNORE 2
#define MGPT_ENVELOPE_MAX_W 2.5f
#define MGPT_ENVELOPE_MAX_RMS 0.1f
#define MGPT_ENVELOPE_PROBE_ROWS 8
#define MGPT_ENVELOPE_PROBE_TOL 1e-5f
#define MGPT_ENVELOPE_PROBE_REL 7.62939453125e-6f      /* 64 * 2^-23 */
int mgpt_gpt_set_envelope_policy(mgpt_gpt *gpt, int policy);
/* out[0] = max|w|, out[1] = max rms(w) over the block matrices (valid after finalize), out[2] = probe error (-1 before the first
 * MGPT_PREC_F16X3 forward under a policy other than IGNORE); *state: 0 not decided yet, 1 inside, 2 outside */
int mgpt_gpt_envelope(mgpt_gpt *gpt, float *out3, int *state);
/* the probe in detail: out[0] = error of the small-call kernels, out[1] = of the large-call kernels (-1 each before the probe),
 * out[2] = the bar they were held to, out[3] = max |logit| of the fp32 path over the probe rows */
int mgpt_gpt_envelope_probe(mgpt_gpt *gpt, float *out4);

/* test/debug: event counters of the policy kernels since the last reset (synchronises the device).
 * which 0 = waves of the C = 256 / C = 160 attention kernels that threw a head of the pipelined key-tile loop (one softmax reference
 * per query and head) away and redid it with the exact running-maximum loop, because a half-row sum of exp2(s - ref) left the
 * fp16 range of the P planes (mapf_gpt_amd/csrc/gpt_kernels_attn_tiles.h).  reset != 0 zeroes the counter after reading it. */
int mgpt_gpt_debug_counter(int which, uint64_t *value, int reset);

/* mgpt_gpt_act with the RNG step read from device memory when the kernel runs (*d_step): for callers that replay the call
 * from a captured hipGraph, where a per-step scalar argument would be frozen */
int mgpt_gpt_act_dev(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, int32_t *d_actions, float *d_logits,
                     int do_sample, uint64_t seed, const uint64_t *d_step, uint64_t row0, int precision, void *stream);

/* ------------------------------------------------------------------------------------------
 * Training (train.py:324-331 with model.py:180-184 and configure_optimizers :202-226), exact fp32 or bf16 mixed precision (train.py's
 * autocast regime, forward_backward_prec), with dropout (model.py:33-34, 59, 66, 71, 82, 88, 129, 175; forward_backward_drop).  Released
 * configs only: bias = False, rows of T = 256 tokens.  In the fp32 path every product is
 * an fp32 fmaf or fp32 MFMA; the bf16 path runs its block linears and attention on bf16 MFMAs with fp32 accumulation.  In both, every reduction
 * runs in a fixed order without floating-point atomics: two identical calls give bit-identical gradients.
 *   train_alloc: workspace for max_rows rows ((12 L + 16) C + 135 + 3 n_head floats per token: 30.1 MB per 6M row, 127.5 MB per 85M
 *           row; one workspace serves both precisions: the bf16 path keeps no weight copies or extra statistics), one fp32 gradient
 *           buffer in the layout of the parameters and the AdamW moments (zeroed), step counters 0.  Needs a
 *           finalized bias = False model (MGPT_ERR_UNSUPPORTED otherwise) with block_size 256 (MGPT_ERR_ARG).  A second call re-sizes the
 *           activation part only (synchronises the device): gradients, moments and step counts are kept.  Nothing is allocated for a model
 *           that never trains.
 *   forward_backward: = forward_backward_prec with MGPT_PREC_F32.
 *   forward_backward_prec: the forward in `precision`, then grads += loss_scale * d(mean cross-entropy, ignore_index = -1)/d(theta); d_targets
 *           int32 [rows][T], -1 = ignored; *d_loss (device, may be NULL) = the unscaled mean loss.  Calls of more rows than the workspace
 *           run in chunks; the mean is over the targeted positions of the whole call.  Synchronises `stream` once, before any other work of
 *           the call is queued, to read the targeted-position count: none (MGPT_ERR_ARG, where torch gives NaN) or a target outside [-1, 67)
 *           (MGPT_ERR_ARG) is refused.  T != 256: MGPT_ERR_ARG.  precision: MGPT_PREC_F32 = the exact-fp32 path above (bit-identical
 *           gradients to forward_backward); MGPT_PREC_BF16 = train.py's torch.amp.autocast(bfloat16) regime: the operands and outputs of the
 *           block linears, q, k, v, attention's output, P and dS and GELU's output are rounded to bf16 (round-to-nearest-even), and the
 *           block linears and attention run on bf16 MFMAs with fp32 accumulation; the embedding, residual stream, LayerNorm, the softmax
 *           statistics, the tied head, cross-entropy,
 *           every accumulator, the gradients and the master weights stay fp32.  The weights are rounded as they are read, so the call
 *           always uses the current parameters and needs no memory beyond the fp32 workspace.  Deterministic like the fp32 path.  Both
 *           precisions accumulate into the same gradient buffer.  Any other precision: MGPT_ERR_UNSUPPORTED.
 *   forward_backward_drop: forward_backward_prec in training mode with dropout probability p at model.py's four places (`sites`, a bit
 *           mask: 1 the embedding sum, 2 the attention probabilities, 4 the output of attention's c_proj, 8 the output of the MLP's c_proj;
 *           15 is the model's behaviour, the other values exist so that a test can name a site).  Stateless, as mgpt_gpt_act is: a mask is
 *           a pure function keep(seed, step, site, layer, element) -- the splitmix64 finaliser over a key of (seed, step) and the stream
 *           (site, layer), counted by the element's index ((row0 + row) * n_head + head) * 65536 + query * 256 + key for the attention
 *           probabilities and ((row0 + row) * 256 + t) * C + c elsewhere, row = the row within the CALL; element e takes bits 16 (e & 3) of
 *           hash(e >> 2), is kept iff they are >= thr = round(p * 65536) and kept values are scaled by 1 / (1 - thr / 65536) in fp32
 *           (restated in mapf_gpt_amd/sampling.py: dropout_keep, dropout_scale).  So a mask does not depend on the workspace size, the
 *           chunking of a call, the precision or the kernel that asks; forward and backward regenerate it, none is stored, and the
 *           workspace is the one above.  The softmax sum runs over all keys, dropped ones included.  In the bf16 path the mask and scale
 *           are applied in fp32 to P and to dP, a branch output is bf16(m s bf16(c_proj)).  p == 0 or sites == 0 runs exactly the launches of
 *           forward_backward_prec; p outside [0, 1) or sites outside [0, 15]: MGPT_ERR_ARG; n_embd not a multiple of 4: MGPT_ERR_UNSUPPORTED.
 *           Deterministic: two identical calls give bit-identical gradients.
 *   forward_backward_rows: the micro-step of rows with ONE targeted position, token 255 (every row the dataset path makes): mathematically
 *           forward_backward_prec(d_tokens, rows, 256, targets) with targets[r][255] = d_labels[r] and -1 elsewhere; d_labels int32 [rows].
 *           The loss is the mean over the `rows` rows of the whole call (chunked like the general call), the gradients accumulate into the
 *           same buffer, and micro-steps of either kind and precision may be mixed within an iteration.  The layers below the last run the
 *           general call's launches; the last layer runs ln_1 and the K | V projection on all tokens and everything else -- the query,
 *           attention's output (attn_last_fwd_kernel), c_proj, the MLP, ln_f, the head, the cross-entropy and their backward
 *           (attn_last_bwd_kernel) -- on the compact matrix of the rows' last tokens, which lives in the activation slots the last layer no
 *           longer fills: the workspace is the one above.  MGPT_PREC_BF16 applies the roundings of the general call at query 255.  NO HOST
 *           WAIT: the normaliser is `rows`, a host-side number, and the call holds no stream synchronise, no blocking copy and no host read
 *           of device memory.  Labels must lie in [0, 67): the cross-entropy kernel compares a label with that range before it indexes
 *           anything with it, and an out-of-range label makes the row's loss term and logit gradients NaN -- *d_loss and the next gradient
 *           norm are NaN, loudly; callers validate on the host where they hold the labels.  No dropout: it is forward_backward_rows_drop
 *           with p = 0 and launches what it launched before that call existed.
 *           Deterministic.  A NULL pointer, rows < 1 or a non-finite loss_scale: MGPT_ERR_ARG; no training workspace: MGPT_ERR_STATE; a
 *           precision other than MGPT_PREC_F32 / MGPT_PREC_BF16: MGPT_ERR_UNSUPPORTED.
 *   forward_backward_rows_drop: forward_backward_rows in training mode with dropout = forward_backward_drop(d_tokens, rows, 256, targets, ...,
 *           p, seed, step, row0, sites) with targets[r][255] = d_labels[r] and -1 elsewhere: the same masks keep(seed, step, site, layer,
 *           element).  The embedding and the layers below the last draw them through the general call's launches; the compact last layer
 *           draws the general call's masks at token / query 255 -- site 1 element ((row0 + row) n_head + head) 65536 + 255 * 256 + key
 *           (attn_last_fwd_kernel / attn_last_bwd_kernel<.., true>), sites 2 and 3 element ((row0 + row) 256 + 255) C + c (the mask's rows
 *           lie 256 C apart, the compact matrix's C).  p, seed, step, row0 and sites as forward_backward_drop takes them, with its refusals
 *           (p outside [0, 1) or sites outside [0, 15]: MGPT_ERR_ARG; n_embd % 4 != 0 with dropout on: MGPT_ERR_UNSUPPORTED); p = 0 or
 *           sites = 0 launches exactly forward_backward_rows.  Everything else is forward_backward_rows' contract: no host wait, the
 *           normaliser `rows`, NaN for an out-of-range label, no floating-point atomics (two identical calls give identical bits), the
 *           same workspace.
 *   zero_grad: grads = 0.
 *   clip_grad_norm: torch.nn.utils.clip_grad_norm_: total = || (||g_p||)_p ||, coef = min(max_norm / (total + 1e-6), 1), g *= coef; the
 *           coefficient stays on the device, *d_total_norm (device, may be NULL) = total.  max_norm <= 0: the norm only.
 *   adamw_step: torch.optim.AdamW with a step count per tensor: p *= 1 - lr * wd (the tensors of dim >= 2 only: wte = lm_head, wpe and the
 *           four matrices of every block), m = lerp(m, g, 1 - beta1), v = beta2 v + (1 - beta2) g^2,
 *           p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).  Afterwards every precision serves the new weights: the
 *           fp32 kernels at once, the 16-bit planes, layer-0 tables and the envelope decision are rebuilt before the next 16-bit call,
 *           and captured step graphs re-capture.
 *   train_get / train_set: one tensor by state_dict key (as mgpt_gpt_set_param; lm_head.weight = transformer.wte.weight) and `which`:
 *           parameter, gradient, exp_avg, exp_avg_sq (the tensor's elements) or the step count (one float).  get copies device to device
 *           on `stream`; set is synchronous (host or device source) and, for a parameter, acts as an optimizer step does on the 16-bit state.
 *           Parameters need no training workspace; the other selectors do (MGPT_ERR_STATE).
 * Data-parallel training (train.py:237-239, 314-322: one process per GPU, gradients averaged over the ranks at an iteration's last
 * micro-step).  No collective runs inside the library: the caller gathers the ranks' buffers ([world][n_elem], rank-major) and the library
 * adds them in rank order, so every rank computes the same bits whatever the collective library's ring or tree would have chosen.
 *   grads_size: *n_elem = the length of the gradient buffer in the library's own layout (the layout of the parameters; padding, if a
 *           layout ever has any, is included, is zero and stays zero).
 *   grads_export: the whole gradient buffer to d_out (device, n_elem floats), an asynchronous device-to-device copy on `stream`.
 *   grads_reduce: d_gathered device float [world][n_elem]; REPLACES the gradient buffer with
 *           scale * (((g[0][i] + g[1][i]) + g[2][i]) + ...): plain fp32 additions in rank order, one multiplication at the end (scale =
 *           1 / world gives DDP's mean).  d_gathered must not overlap the gradient buffer.  16-byte loads and stores when d_gathered is
 *           16-byte aligned and n_elem % 4 == 0, element by element otherwise; no atomics.
 *   All three: a NULL pointer or a wrong n_elem MGPT_ERR_ARG; world < 1 or a scale that is not finite and positive MGPT_ERR_ARG; no
 *           training workspace MGPT_ERR_STATE.
 * ------------------------------------------------------------------------------------------ */
#define MGPT_TRAIN_PARAM 0
#define MGPT_TRAIN_GRAD 1
#define MGPT_TRAIN_EXP_AVG 2
#define MGPT_TRAIN_EXP_AVG_SQ 3
#define MGPT_TRAIN_STEP 4
int mgpt_gpt_train_alloc(mgpt_gpt *gpt, int max_rows);
int mgpt_gpt_train_free(mgpt_gpt *gpt);
int mgpt_gpt_forward_backward(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, int T, const int32_t *d_targets, float loss_scale,
                              float *d_loss, void *stream);
int mgpt_gpt_forward_backward_drop(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, int T, const int32_t *d_targets, float loss_scale,
                                   float *d_loss, int precision, float p, uint64_t seed, uint64_t step, uint64_t row0, int sites, void *stream);
int mgpt_gpt_forward_backward_prec(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, int T, const int32_t *d_targets, float loss_scale,
                                   float *d_loss, int precision, void *stream);
int mgpt_gpt_forward_backward_rows(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, const int32_t *d_labels, float loss_scale, float *d_loss,
                                   int precision, void *stream);
int mgpt_gpt_forward_backward_rows_drop(mgpt_gpt *gpt, const uint8_t *d_tokens, int rows, const int32_t *d_labels, float loss_scale, float *d_loss,
                                        int precision, float p, uint64_t seed, uint64_t step, uint64_t row0, int sites, void *stream);
int mgpt_gpt_zero_grad(mgpt_gpt *gpt, void *stream);
int mgpt_gpt_clip_grad_norm(mgpt_gpt *gpt, float max_norm, float *d_total_norm, void *stream);
int mgpt_gpt_adamw_step(mgpt_gpt *gpt, float lr, float beta1, float beta2, float eps, float weight_decay, void *stream);
int mgpt_gpt_train_get(mgpt_gpt *gpt, const char *name, int which, float *d_out, int64_t n_elem, void *stream);
int mgpt_gpt_train_set(mgpt_gpt *gpt, const char *name, int which, const float *data, int64_t n_elem, int is_device);
int mgpt_gpt_grads_size(mgpt_gpt *gpt, int64_t *n_elem);
int mgpt_gpt_grads_export(mgpt_gpt *gpt, float *d_out, int64_t n_elem, void *stream);
int mgpt_gpt_grads_reduce(mgpt_gpt *gpt, const float *d_gathered, int world, float scale, void *stream);

/* sampling alone (same RNG and key as mgpt_gpt_act), for callers that already hold logits */
int mgpt_sample_actions(const float *d_logits, int rows, int32_t *d_actions, int do_sample,
                        uint64_t seed, uint64_t step, uint64_t row0, void *stream);
/* The same on the COMPACT logits of a subset of the instances (the sampler of the step object's retire mode, below): d_live int32 holds
 * the ids of the chosen instances, *d_count (device int32) how many; compact row j of d_logits [*d_count * n_agents, 67] belongs to
 * instance d_live[j / n_agents], agent j % n_agents.  Its action goes to d_actions[d_live[j / n_agents] * n_agents + j % n_agents] and its
 * draw is keyed by row0 + that index: every chosen row gets what mgpt_sample_actions gives it on the full logits.  Other entries of
 * d_actions are not written.  The count is read on the device: no synchronisation. */
int mgpt_sample_actions_live(const float *d_logits, const int32_t *d_live, const int32_t *d_count, int n_agents, int32_t *d_actions,
                             int do_sample, uint64_t seed, uint64_t step, uint64_t row0, void *stream);
/* Ordered list of the instances that are not done: d_done uint8 [n_inst] (mgpt_env_state) -> d_live int32 [n_inst]: the indices i with
 * d_done[i] == 0 in ascending order, then -1; *d_count (device int32) = how many.  A stable stream compaction in one workgroup (wave
 * ballots, an LDS pass over the wave totals), no atomics: the same flags give the same bits.  n_inst >= 1. */
int mgpt_live_list(const uint8_t *d_done, int n_inst, int32_t *d_live, int32_t *d_count, void *stream);

/* ------------------------------------------------------------------------------------------
 * One whole environment step = the body of the reference's episode loop (example.py:63-65 around
 * inference.py:151-172):  update_agents(pos, goal, last actions) -> generate_observations -> act -> env.step.
 * The launch sequence is static, so after one eager step it is captured as a hipGraph and replayed: one call, no
 * per-launch host cost.  The contexts stay owned by the caller and must outlive the step object.
 *   create: rows = n_inst * n_agents of the tokenizer/env pair; precision / do_sample / seed / row0 as in mgpt_gpt_act.
 *   run:    d_tokens uint8 [rows, 256] scratch (holds this step's observation rows afterwards); d_actions int32 [rows]
 *           IN: the previous intended actions (-1 on the first step, inference.py:140), OUT: this step's actions, already
 *           executed by the env.  goals_may_change as in mgpt_tokenizer_update_agents.  use_graph = 0 forces eager launches
 *           (identical results); eager is also used while the timing hooks are enabled.
 *   reset:  sets the RNG step counter (call with 0 when an episode starts; the k-th run after it draws with step k) and
 *           drops the captured graph -- call it after anything that re-allocates inside the contexts (mgpt_env_set_lifelong).
 *           In retire mode it also makes every instance live again.
 * Retire mode (opt-in): the reference's run_episode leaves an episode when all agents are terminated or truncated (create_env.py:15-18);
 * a batch keeps stepping, but the policy -- about 99 % of a step -- need not see the finished instances.
 *   set_retire: enable != 0 allocates an ordered list of live instance ids, its count (device int32 + a pinned host int32), a compact
 *           token buffer [rows, 256] and compact logits [rows, 67]; every instance starts live.  enable == 0 frees them and restores the
 *           plain step exactly.  Synchronous.
 *   poll_live:  mgpt_live_list on the env's done flags, the count copied to the pinned int, `stream` synchronised, the count returned in
 *           *n_live (may be NULL).  The only host synchronisation of the mode.  Between polls the list and the policy's row count are
 *           FROZEN: an instance that finishes inside the window is forwarded until the next poll, which changes nothing, because the env
 *           ignores the actions of a done instance.
 *   run in retire mode: update_agents and generate_observations on ALL rows (d_tokens holds the full batch's rows, as ever), a gather of
 *           the live instances' rows, the forward on those n_live * n_agents rows (the call regime follows that row count, as for any
 *           call), mgpt_sample_actions_live into d_actions -- the entries of retired instances keep their last value --, env.step, the
 *           step-counter bump.  With no live instance the gather, the forward and the sampler are skipped.  Draws are keyed by the global
 *           row, so the MGPT_PREC_F32 kernels, which compute a row from that row alone, give every live row the bits of the plain step;
 *           the 16-bit paths pick different kernels at <= 128 and above 128 rows, so a compacted call can differ from the plain one in the
 *           last bits of a logit (within the envelope's bar).  use_graph != 0: MGPT_ERR_UNSUPPORTED (the row count changes).
 *           d_tokens must be 16-byte aligned.
 *   copy_live:  test/debug: the live list (int32 [n_inst]) and the compact logits of the last run (float32 [rows, 67], the first
 *           n_live * n_agents rows valid) into caller-owned device buffers; either may be NULL.
 * Episode recorder (opt-in): the trajectory of the policy's own episode stays on the device.
 *   set_record: enable != 0 allocates, for T = the env's max_episode_steps, traj_pos int16 [T + 1][rows][2], traj_act int8 [T][rows] and
 *           a one-word device t0 (zero-filled; t0 = the current step counter), and drops a captured graph.  enable == 0 frees them and
 *           restores the plain step exactly.  Synchronous.
 *   reset with recording on: t0 = step0, both buffers zero-filled, the env's current positions copied into slot 0 -- so the env must
 *           have been reset BEFORE mgpt_step_reset (mgpt_env_reset, then mgpt_step_reset: the order BatchedRunner.reset calls in).
 *   run with recording on: one more launch (timing-hook name step_record) after the env step (and the shield's commit), before the
 *           counter bump: with t = step counter - t0 read on the device, traj_pos[t + 1][row] = the row's position after the step and
 *           traj_act[t][row] = (int8) the action handed to the env (with a shield: the planned one), for every row, done or retired
 *           instances included (they do not move; their action entries beyond the episode's length -- the env's ep_length metric --
 *           mean nothing).  A step with t >= T writes nothing.  Eager, graph, retire, shield and lifelong steps all record.
 *   copy_record: traj_pos and traj_act into caller-owned device buffers of those shapes; either may be NULL.  MGPT_ERR_STATE with
 *           recording off.
 * ------------------------------------------------------------------------------------------ */
typedef struct mgpt_step mgpt_step;
int mgpt_step_create(mgpt_step **out, mgpt_tokenizer *tok, mgpt_gpt *gpt, mgpt_env *env, int rows, int precision,
                     int do_sample, uint64_t seed, uint64_t row0);
int mgpt_step_destroy(mgpt_step *step);
int mgpt_step_reset(mgpt_step *step, uint64_t step0, void *stream);
int mgpt_step_run(mgpt_step *step, uint8_t *d_tokens, int32_t *d_actions, int goals_may_change, int use_graph, void *stream);
int mgpt_step_set_retire(mgpt_step *step, int enable);
int mgpt_step_poll_live(mgpt_step *step, int *n_live, void *stream);
int mgpt_step_copy_live(mgpt_step *step, int32_t *d_live_out, float *d_logits_out, void *stream);
int mgpt_step_set_record(mgpt_step *step, int enable);
int mgpt_step_copy_record(mgpt_step *step, int16_t *d_pos_out, int8_t *d_act_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Dataset-side bulk tokenizer: replaces dataset/tokenizer/generate_observations.py:8-92 with its two native modules
 * (cost2go.cpp:33-88 precompute_cost2go / generate_cost2go_obs, encoder.cpp:88-127 Encoder::encode) -- every
 * (agent, timestep) of a logged episode becomes one 256-token row.
 *   create:   d_grid uint8 [H][W] PADDED map (non-zero = blocked); builds the all-pairs BFS table of the map
 *             (= the reference's cost2go_data dict, cached per map_name at :47-54).  Synchronises `stream` once.
 *   tokenize: d_paths int16 [n_agents][n_steps][2] = cells visited (padded coords, get_agent_paths :159-177; the goal of an
 *             agent is its last cell); d_tokens uint8 [n_agents][n_steps][256], agent-major like the reference's append
 *             order (:70-90).  Lifelong logs (per-step goals, :55-60) are not supported.  Relative goals beyond +-20 are
 *             clamped (the reference's unordered_map::at throws there).
 * ------------------------------------------------------------------------------------------ */
typedef struct mgpt_dataset mgpt_dataset;
int mgpt_dataset_create(mgpt_dataset **out, const uint8_t *d_grid, int H, int W, void *stream);
int mgpt_dataset_destroy(mgpt_dataset *ds);
int mgpt_dataset_tokenize(mgpt_dataset *ds, int n_agents, int n_steps, const int16_t *d_paths, uint8_t *d_tokens, void *stream);
/* the same with the two options of the reference's generator:
 *   d_goals  int16 [n_agents][n_steps][2] or NULL: lifelong logs (generate_observations.py:55-60,143-153) -- the goal every
 *            agent pursued at every timestep (relative goal + greedy-direction bits of its records); the cost-to-go window
 *            stays that of the path's last cell, as in the reference (:75-78);
 *   only_obstacles != 0: the mask_cost2go ablation (cost2go.cpp:52-62) -- window cells become the integers 0 / 1 (blocked). */
int mgpt_dataset_tokenize_ex(mgpt_dataset *ds, int n_agents, int n_steps, const int16_t *d_paths, const int16_t *d_goals,
                             int only_obstacles, uint8_t *d_tokens, void *stream);
/* A batch of episodes of one map, straight from the expert's device log: no per-episode host work.
 *   d_init     int16 [n_batch][n_agents][2]: the agents' first cells, padded coords (the table's frame);
 *   d_actions  int8 [n_batch][n_agents][max_steps]: the made actions, the layout of mgpt_expert_copy_log.  A byte outside 0..4 counts as
 *              a wait; cells are clamped into the frame, so no byte value moves a read out of bounds (a logged path never leaves it);
 *   d_len      int32 [n_batch]: actions made per episode, clamped to [0, max_steps] on the device;
 *   d_keep     uint8 [n_batch] or NULL: 0 = the episode gives no rows (generate_observations.py:44-45, CSR < 1);
 *   d_episodes int32 [n_sel] or NULL: the selected episodes (indices below n_batch, any order, repeats allowed); NULL = 0 .. n_sel - 1.
 *   episode_offsets:   d_row0 int64 [n_sel + 1] = the exclusive scan of rows(k) = keep ? n_agents * (len + 1) : 0 in selection order.  One
 *              workgroup, no atomics: the same bits on every run.
 *   tokenize_episodes: d_row0 as episode_offsets wrote it for the same arguments, or a window of n_sel + 1 entries of a longer scan together
 *              with the same window of d_episodes (not NULL then): a large selection is tokenized in several calls into one output.
 *              Rows [row0[k], row0[k + 1]) of d_tokens uint8 [N][256] and d_labels int8 [N] (N = the scan's last entry) are what
 *              mgpt_dataset_tokenize makes of the episode's paths (init + the running sum of the moves; the goal is the path's last
 *              cell), agent-major then timestep 0 .. len, and the labels of generate_observations.py:67-90: with a = actions[:len] +
 *              [0] and g the index of a's last non-zero entry (len + 1 if none), 5 where t > g, else a[t].  Lifelong logs (per-step
 *              goals) go through mgpt_dataset_tokenize_episodes_lifelong below.  Stream-ordered; no host synchronisation except
 *              when the context's workspace (16 bytes per row of n_sel * n_agents * (max_steps + 1)) grows.  MGPT_ERR_UNSUPPORTED
 *              when that product reaches 2^31: split the selection.  n_sel = 0 launches nothing. */
int mgpt_dataset_episode_offsets(int n_sel, int n_agents, int max_steps, const int32_t *d_len, const uint8_t *d_keep,
                                 const int32_t *d_episodes, int64_t *d_row0, void *stream);
int mgpt_dataset_tokenize_episodes(mgpt_dataset *ds, int n_sel, int n_agents, int max_steps, const int16_t *d_init, const int8_t *d_actions,
                                   const int32_t *d_len, const uint8_t *d_keep, const int32_t *d_episodes, const int64_t *d_row0,
                                   int only_obstacles, uint8_t *d_tokens, int8_t *d_labels, void *stream);
/* The same for LIFELONG logs (generate_observations.py:55-60, 72-79, 156-166, 188-202): the arguments of
 * tokenize_episodes plus the agents' target lists.  An agent's list is target(0), target(1), ...; walking its path t = 0 .. len with
 * cur = 0, a cell equal to target(cur) advances cur by one (an `if`, not a loop; also at t = 0, before that cell's goal is read) and the
 * goal at t is target(cur).  The record of every agent (own and neighbours) carries that per-step goal -- the relative goal and the
 * greedy-direction bits of the goal's field; the cost-to-go window is still cut from the field of the path's LAST CELL, as in the
 * reference (:75-78).  Labels, history, row order and offsets are those of tokenize_episodes.
 *   d_targets   int16 [n_batch][n_agents][L][2], L >= 1: target(0) = entry 0 and, for j >= 1, target(j) = entry 1 + (j - 1) % (L - 1) --
 *               the expert's (goal at reset, cyclic queue of Q = L - 1) as it lies; a plain list is the case without a wrap;
 *   d_n_targets int32 [n_batch][n_agents] or NULL (= L each): the length of every list, j < n_targets;
 *   d_status    int32 [1], zeroed by the caller: set to 1 (a plain store, stream-ordered) when a kept agent's walk reaches n_targets
 *               or n_targets < 1 -- the reference's IndexError.  The walk goes on with the last valid index: the rows of such a call are
 *               unspecified, every access stays in bounds.
 * A target outside the frame gives no table read and the direction bits "0000", as an out-of-frame goal of tokenize_ex; init cells and
 * moves are clamped as in tokenize_episodes: no byte of d_init, d_actions, d_targets or d_n_targets moves a read out of bounds.  Same
 * stream ordering, workspace (plus 4 bytes per n_sel * n_agents), windows of a longer scan and n_sel = 0 rule as tokenize_episodes. */
int mgpt_dataset_tokenize_episodes_lifelong(mgpt_dataset *ds, int n_sel, int n_agents, int max_steps, const int16_t *d_init,
                                            const int8_t *d_actions, const int32_t *d_len, const uint8_t *d_keep, const int32_t *d_episodes,
                                            const int64_t *d_row0, const int16_t *d_targets, int L, const int32_t *d_n_targets,
                                            int32_t *d_status, int only_obstacles, uint8_t *d_tokens, int8_t *d_labels, void *stream);

/* ------------------------------------------------------------------------------------------
 * Dataset builder: steps 2-3 of dataset/generate_dataset.py on rows that the bulk tokenizer above has left on the device --
 * balance_and_filter_tensors (:65-103; sha256 of every row into a python set, then the "wait in goal" balancing loop) and the
 * index arithmetic of its shuffles and picks.  Rows are uint8 [n][256] (16-byte aligned), labels int8 [n] in 0..5.
 *   dedup_create:  a set for up to capacity_rows (<= 2^28) distinct rows: an open-addressing table (the power of two >= 2 x capacity
 *           slots), the rows themselves and per-call workspace (about 300 bytes per row of capacity in all).  hash_bits 1 .. 64
 *           masks the row hash: 64 in production, small values make tests collide.  Anything else: MGPT_ERR_ARG.
 *   dedup_reset:   empties the set (stream-ordered).
 *   dedup_count:   rows in the set (host value, no synchronisation).
 *   dedup_filter:  d_first[i] = 1 iff no row of the set and no row j < i of the batch has the same 256 bytes; those rows join the
 *           set.  The answer is exact whatever the hash does (rows that share a hash are compared byte by byte) and the same bits
 *           on every run.  d_counts (device, may be NULL) int64 [4] = {first occurrences, duplicates, rows that shared a hash with a
 *           different row, rows in the set afterwards}.  MGPT_ERR_ARG, before any state changes, when the set's rows + n exceed the
 *           capacity.  MGPT_ERR_UNSUPPORTED when more rows collide than the exact pass takes (65536 per call, 4096 distinct ones
 *           per set: not reachable with 64-bit hashes); the set is then unusable until reset (MGPT_ERR_STATE).  Synchronises
 *           `stream` once to read the counts.
 *   rows_workspace_bytes: size of the d_work buffer (16-byte aligned) that dataset_balance and rows_select want for n rows.
 *   dataset_balance: the balancing loop of :80-95 in closed form over the rows with d_first != 0: with their count N, z = #(label 0) +
 *           #(label 5) and n5 = #(label 5), k is the smallest value with k == n5 or z - k <= (N - k) / 5; the k label-5 rows of highest
 *           index are dropped (d_keep = 0), every label 5 becomes 0 in d_labels_out (written for all n rows).  d_stats int64 [10] =
 *           {discarded, duplicates (n - N), kept, actions_made[0..5] as the reference prints them (:96), labels outside 0..5}.
 *   rows_select:  d_index = the positions of the non-zero bytes of d_keep in increasing order, *d_count = how many (both device; d_index
 *           holds up to n entries).  Counting, a scan and a scatter: no atomics.
 *   rows_gather:  d_rows_out[r] = d_rows[d_index[r]], d_labels_out[r] = d_labels[d_index[r]] (labels optional) for r < n_out; an index
 *           outside [0, n_src) gives a zero row with label -1.
 * ------------------------------------------------------------------------------------------ */
typedef struct mgpt_dedup mgpt_dedup;
int mgpt_dedup_create(mgpt_dedup **out, int64_t capacity_rows, int hash_bits, void *stream);
int mgpt_dedup_destroy(mgpt_dedup *set);
int mgpt_dedup_reset(mgpt_dedup *set, void *stream);
int mgpt_dedup_count(const mgpt_dedup *set, int64_t *rows);
int mgpt_dedup_filter(mgpt_dedup *set, const uint8_t *d_rows, int64_t n, uint8_t *d_first, int64_t *d_counts, void *stream);
int mgpt_rows_workspace_bytes(int64_t n, int64_t *bytes);
int mgpt_dataset_balance(const uint8_t *d_first, const int8_t *d_labels, int64_t n, uint8_t *d_keep, int8_t *d_labels_out,
                         int64_t *d_stats, void *d_work, void *stream);
int mgpt_rows_select(const uint8_t *d_keep, int64_t n, int64_t *d_index, int64_t *d_count, void *d_work, void *stream);
int mgpt_rows_gather(const uint8_t *d_rows, const int8_t *d_labels, int64_t n_src, const int64_t *d_index, int64_t n_out,
                     uint8_t *d_rows_out, int8_t *d_labels_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * PIBT expert: the role of run_expert() (dataset/generate_dataset.py:214-230) and of the logging environment
 * (experiment_setup/create_env.py:8-33: create_logging_env, LogActions :49-60) -- plans every agent's next cell by priority inheritance
 * with backtracking (the spec is this project's own: DESIGN.md section 20; the reference's expert is LaCAM3, which is not rebuilt), steps
 * the env with the plan and logs the actions made.  A weaker teacher than LaCAM: nothing guarantees that all agents reach their goals.
 *   create:    borrows the distance fields and grids of `tok` (mgpt_tokenizer_create_agents must have run before the first reset) and
 *              pos / goal / done of `env`; both must outlive the expert and agree in shape (MGPT_ERR_ARG otherwise).  seed and
 *              inst_offset key the tie-breaking draws by the GLOBAL row (inst_offset + inst) * n_agents + agent, so a shard plans what the
 *              unsharded job plans.  max_steps = the log's capacity per agent.  MGPT_ERR_UNSUPPORTED for a lifelong env, for a non-zero env
 *              rule mask (also when either is set later: reset and step check again) and for n_agents > 65534 (generate_dataset.py:214-230).
 *   reset:     since = 0, empty log, empty occupancy (every plan rebuilds it from the env's positions); call after mgpt_env_reset and
 *              mgpt_tokenizer_create_agents (create_env.py:8-33).
 *   step:      plan -> log -> mgpt_env_step -> since update, one call (generate_dataset.py:214-230).  d_actions int32 [n_inst, n_agents]
 *              OUT: the planned actions, already executed by the env.  Instances that are done get action 0 and log nothing.
 *   copy_plan: test read-back, int16 [n_inst, n_agents, 2]: the cell every agent planned to stand on after the last step
 *              (create_env.py:8-33).
 *   copy_log:  the made actions int8 [n_inst][n_agents][max_steps] and their count per instance int32 [n_inst] (= the instance's
 *              ep_length); either may be NULL (create_env.py:8-33 LogActions; generate_dataset.py:214-230).
 * ------------------------------------------------------------------------------------------ */
typedef struct mgpt_expert mgpt_expert;
int mgpt_expert_create(mgpt_expert **out, mgpt_tokenizer *tok, mgpt_env *env, uint64_t seed, int64_t inst_offset, int max_steps);
int mgpt_expert_destroy(mgpt_expert *ex);
int mgpt_expert_reset(mgpt_expert *ex, void *stream);
int mgpt_expert_step(mgpt_expert *ex, int32_t *d_actions, void *stream);
int mgpt_expert_copy_plan(mgpt_expert *ex, int16_t *d_planned_out, void *stream);
int mgpt_expert_copy_log(mgpt_expert *ex, int8_t *d_log_out, int32_t *d_len_out, void *stream);

/* LaCAM search over the PIBT generator (plain depth-first LaCAM, Okumura AAAI 2023, restated over section 20's
 * step; nothing is taken from the reference's dataset/lacam).  Without set_search every call above behaves as it did.
 *   set_search:    allocates the per-instance node store, open stack, constraint pool and hash table for at most max_iters iterations
 *                  (1 .. 2^24).  iters_per_launch: iterations per instance and launch, 0 = the library's default.  hash_bits: 0 = the table's
 *                  own size; 1 .. 63 cuts the hash to that many bits before the probe starts (tests: every lookup then goes through the
 *                  equality check; the outcome does not change).  May be called again; MGPT_ERR_ARG for values out of range.
 *   solve:         right after mgpt_expert_reset (MGPT_ERR_STATE otherwise, or without set_search): searches every instance from the env's
 *                  positions; launches until no instance is unfinished, reading one device counter per launch (synchronises the stream).
 *   copy_search:   int32 [n_inst] each, any may be NULL: status (1 solved within max_steps, 2 open ran empty: no solution exists,
 *                  3 max_iters reached, 4 solved but longer than max_steps), iterations used, nodes created, solution length (0 unless
 *                  status is 1 or 4).
 *   copy_solution: int8 [n_inst][n_agents][max_steps]: the actions of the status-1 instances, 0 elsewhere.
 *   step:          in search mode (after solve; MGPT_ERR_STATE before it) a status-1 instance replays its solution -- actions, planned
 *                  cells and log come from it -- and every other instance is planned by PIBT as before.
 */
int mgpt_expert_set_search(mgpt_expert *ex, int max_iters, int iters_per_launch, int hash_bits);
int mgpt_expert_solve(mgpt_expert *ex, void *stream);
int mgpt_expert_copy_search(mgpt_expert *ex, int32_t *d_status, int32_t *d_iters, int32_t *d_nodes, int32_t *d_length, void *stream);
int mgpt_expert_copy_solution(mgpt_expert *ex, int8_t *d_solution_out, void *stream);

/* Corridor swap rule in the generator (the swap technique of Okumura, IJCAI 2023, restated over section 20's
 * candidates; nothing is taken from the reference's dataset/lacam).  Off by default: without it every call above behaves as it did.
 *   set_swap:  on = 1 turns the rule on in the plan kernel and in the search's generator (whichever of set_search and set_swap comes
 *              first), on = 0 turns it off again; any other value is MGPT_ERR_ARG.  Allowed before mgpt_expert_reset, right after it
 *              (before solve and the first step) and between episodes, i.e. once every instance is done (this call reads the done flags:
 *              it synchronises the device); MGPT_ERR_STATE in the middle of an episode.  The first on = 1 builds a degree map of the
 *              grids (timing-hook name expert_cell_degree) that the context keeps.  MGPT_ERR_UNSUPPORTED when the frames with their swap
 *              agents (2 more bytes of LDS per agent) do not fit.
 */
int mgpt_expert_set_swap(mgpt_expert *ex, int on);

/* Refinement of found solutions by single-agent space-time replanning (this project's own spec in the place of
 * the anytime refinement of LaCAM3, the reference's expert, which is not in its tree: generate_dataset.py:214-230 only calls it;
 * nothing is taken from the reference's dataset/lacam).  Off by default: without it every call above behaves as it did.
 *   set_refine:    after mgpt_expert_set_search (MGPT_ERR_STATE without it; a later set_search turns the pass off again), before
 *                  mgpt_expert_reset or between episodes (MGPT_ERR_STATE in the middle of one; reads the done flags as set_swap does).
 *                  max_rounds 1 .. 65536 turns the pass on and sizes its memory, 0 turns it off and frees it.  horizon: solutions of
 *                  up to this many steps are refined, 0 = twice max_steps, otherwise max_steps .. 2^20; MGPT_ERR_ARG outside these.
 *                  MGPT_ERR_UNSUPPORTED when the horizon + 1 reach layers of the map do not fit the 160 KiB of LDS of a workgroup.
 *   solve:         with the pass on, every instance the search left with status 1 or 4 and a length within the horizon is refined:
 *                  rounds in which every agent is replanned once against the others' paths, until a round adopts nothing or max_rounds
 *                  have run (one device counter read per round: synchronises the stream; timing-hook names expert_refine_path,
 *                  expert_refine_round, expert_refine_final).
 *   copy_search:   status and length are then the FINAL ones, which the episode replays (a status-4 instance may have become 1);
 *                  iterations and nodes are the search's.  copy_solution returns the refined solution.
 *   copy_refine:   int32 [n_inst] each, any may be NULL: the search's own status and length, the sum of costs before and after, rounds
 *                  run, replans adopted (the last four are 0 for an instance that was left as it is).  MGPT_ERR_STATE before a solve or
 *                  with the pass off.
 */
int mgpt_expert_set_refine(mgpt_expert *ex, int max_rounds, int horizon);
int mgpt_expert_copy_refine(mgpt_expert *ex, int32_t *d_first_status, int32_t *d_first_length, int32_t *d_soc_before, int32_t *d_soc_after,
                            int32_t *d_rounds, int32_t *d_replans, void *stream);

/* Lifelong episodes (on_target = restart; DESIGN.md section 30: section 20's plan on goals that move, the role of run_expert() on the
 * reference's lifelong env, create_env.py:28-32).  Off by default: without it every call above behaves as it did, the refusal of a
 * lifelong env included.
 *   set_lifelong:  on = 1 / 0, any other value is MGPT_ERR_ARG.  Before mgpt_expert_reset or between episodes (MGPT_ERR_STATE in the middle
 *                  of one; reads the done flags as set_swap does); a reset must follow before the next step.  MGPT_ERR_UNSUPPORTED together
 *                  with the search in either order (set_search, and set_refine with it, look for a joint goal configuration).  The order of
 *                  calls is create (on an env that is not lifelong yet), set_lifelong(1), mgpt_env_set_lifelong, the resets.
 *   reset / step:  with it on the env must be lifelong: MGPT_ERR_STATE otherwise (mgpt_env_set_lifelong must come first).  A step is
 *                  plan -> log -> mgpt_env_step -> mgpt_tokenizer_update_agents(goals_may_change = 1) on the borrowed tokenizer, fed the
 *                  actions just made, which rebuilds the distance field of every agent whose goal changed -> the post-step kernel
 *                  (timing-hook name expert_lifelong_post): since = 0 for an agent whose new cell is the goal it pursued during the step
 *                  (the env's own arrival test), else since + 1, and the arrivals of the step.  Episodes end by truncation only.
 *   copy_arrivals: int16 [n_inst][max_steps]: arrivals per instance and step (0 beyond the steps made); their sum over an episode is the
 *                  sum over the agents of mgpt_env_lifelong_counts.  MGPT_ERR_STATE with lifelong planning off or before a reset.
 */
int mgpt_expert_set_lifelong(mgpt_expert *ex, int on);
int mgpt_expert_copy_arrivals(mgpt_expert *ex, int16_t *d_arrivals_out, void *stream);

/* Collision shield (section 20's PIBT with the policy's action preferences as every agent's candidate order, "CS-PIBT"
 * of Veerapaneni et al., ICAPS 2024, restated over this project's own spec).  Off by default: without it every call above behaves as it did.
 *   set_shield:    on = 1 / 0, any other value is MGPT_ERR_ARG.  on = 1 allocates `first` [n_inst][n_agents] and `overrides` [n_inst]; a reset
 *                  must follow.  MGPT_ERR_UNSUPPORTED together with set_search, set_swap, set_refine or set_lifelong (in either order), for a
 *                  lifelong env and for a non-zero env rule mask.  MGPT_ERR_STATE in the middle of an episode (reads the done flags as
 *                  set_swap does, and a device flag that every shield launch sets and reset clears: steps replayed from a captured
 *                  graph count).  On a shield-mode context mgpt_expert_step and mgpt_expert_solve return MGPT_ERR_STATE.
 *   shield:        plans only (timing-hook name expert_shield).  d_actions int32 [n_inst, n_agents] IN: the sampler's action of every row
 *                  (`first`, kept as a copy), OUT: the planned actions.  d_logits: float32 rows of ld >= 5 values, the first five are read.
 *                  An agent's candidates are tried with `first` first, the others by descending logit (compared as bit patterns: the fp32
 *                  pattern mapped monotonically to u32, so -0 < +0 and NaNs have a fixed place), ties by ascending action.  d_live = NULL
 *                  (d_count NULL too): every instance, the logits of instance i at rows i * n_agents ...  Otherwise block b < *d_count
 *                  handles instance d_live[b] with its logits at rows b * n_agents ..; d_actions is indexed by the global row in both
 *                  modes.  Instances that are done, or not in the live list, are left untouched.  overrides[i] grows by the agents of
 *                  instance i whose planned action is not `first`.
 *   shield_commit: the since update of section 20; call after mgpt_env_step has executed the planned actions.
 *   copy_shield:   int32 [n_inst, n_agents] `first` of the last shield call and int32 [n_inst] overrides since reset; either may be NULL.
 *                  mgpt_expert_copy_plan gives the planned cells.
 * In the step (mgpt_step above):
 *   step_set_shield: attaches a shield-mode expert made from the step's own tokenizer and env contexts (MGPT_ERR_ARG otherwise;
 *                  MGPT_ERR_STATE for an expert that is not in shield mode); NULL detaches.  Allocates a logits buffer [rows][67] for the
 *                  plain path and drops a captured graph.  A run is then update_agents -> generate_observations -> act (logits kept) ->
 *                  shield -> env.step -> shield_commit -> the counter bump; d_actions holds the planned actions, which are the made ones,
 *                  and the next run's update_agents sees them.  The launch sequence stays static: use_graph works as before.  The caller
 *                  resets the expert (mgpt_expert_reset) whenever it resets the step.
 *   step_copy_shield_logits: test read-back of the plain path's logits of the last run, float32 [rows][67] (retire mode:
 *                  mgpt_step_copy_live).  MGPT_ERR_STATE without an attached shield.
 */
int mgpt_expert_set_shield(mgpt_expert *ex, int on);
int mgpt_expert_shield(mgpt_expert *ex, const float *d_logits, int64_t ld, const int32_t *d_live, const int32_t *d_count, int32_t *d_actions,
                       void *stream);
int mgpt_expert_shield_commit(mgpt_expert *ex, void *stream);
int mgpt_expert_copy_shield(mgpt_expert *ex, int32_t *d_first_out, int32_t *d_overrides_out, void *stream);
int mgpt_step_set_shield(mgpt_step *step, mgpt_expert *ex);
int mgpt_step_copy_shield_logits(mgpt_step *step, float *d_out, void *stream);

/* The collision shield on lifelong episodes (on_target = restart; DESIGN.md section 35: section 31's plan on the fields of the goals the
 * agents hold now, section 30's rules after the env step).  Off by default: without it every call above behaves as it did, the shield's
 * refusal of a lifelong env and of set_lifelong included.
 *   set_shield_lifelong: on = 1 / 0, any other value is MGPT_ERR_ARG.  On a shield-mode context only (MGPT_ERR_STATE otherwise), before
 *                  mgpt_expert_reset or between episodes (MGPT_ERR_STATE in the middle of one, read from the device as set_shield does).
 *                  on = 1 allocates `held` u32 [n_inst][n_agents], `live` u8 [n_inst], `arrivals` int16 [n_inst][max_steps] and `steps`
 *                  int32 [n_inst]; 0 frees them and restores the plain shield; mgpt_expert_set_shield(ex, 0) releases them too.  A reset
 *                  must follow.  The order of calls is create (on an env that is not lifelong yet), set_shield(1), set_shield_lifelong(1),
 *                  mgpt_env_set_lifelong, the resets.
 *   reset / shield: with it on the env must be lifelong: MGPT_ERR_STATE otherwise (mgpt_env_set_lifelong must come first).  reset copies
 *                  the env's goals into `held`, sets `live` and clears `arrivals` and `steps`.
 *   shield_commit: launches the post-step kernel (timing-hook name expert_shield_lifelong_post) in the since update's place: since = 0 for
 *                  an agent whose new cell is the goal it held during the step, else since + 1; held = the env's goals; the arrivals of the
 *                  step go to arrivals[inst][steps[inst]] while that index is below max_steps, and steps[inst] grows by one -- no argument
 *                  changes from step to step, so a captured step replays it.  It never calls the tokenizer: the distance fields of the
 *                  agents whose goal changed are rebuilt by the caller, once per step and before the next plan, with
 *                  mgpt_tokenizer_update_agents(goals_may_change = 1) -- in mgpt_step_run that is the update at the head of the next run;
 *                  a caller that drives shield / env_step / shield_commit itself issues it between the env step and the commit.
 *   copy_arrivals: mgpt_expert_copy_arrivals serves this mode as well.
 */
int mgpt_expert_set_shield_lifelong(mgpt_expert *ex, int on);

/* ------------------------------------------------------------------------------------------
 * Kernel timing hooks (bench.py's live roofline): when enabled, the library brackets every kernel
 * class with hipEvents on the launch stream.  mgpt_prof_read synchronises the device.
 * ------------------------------------------------------------------------------------------ */
#define MGPT_PROF_MAX 64
int mgpt_prof_enable(int on);
int mgpt_prof_reset(void);
/* names[i] (static strings), total_ms[i], launches[i] for i < *n (n in: capacity, out: used) */
int mgpt_prof_read(const char **names, float *total_ms, int64_t *launches, int *n);

#ifdef __cplusplus
}
#endif
#endif /* MAPF_GPT_AMD_H */
