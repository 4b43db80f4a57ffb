// gpt_ctx.h -- policy context shared by the fp32 and the fast (16-bit MFMA) forward paths.
#pragma once
#include <vector>

#include "common.h"
#include "gpt_plan.h"      // kSmallRows, and the launch plan of the 16-bit forward (host-only)

struct LayerOff {
    size_t ln1, attn_w, proj_w, ln2, fc_w, proj2_w;
};

// GPTConfig.bias = True (model.py:14-17,29,31,79,81,115): LayerNorm and Linear bias vectors, offsets into mgpt_gpt::bias
struct BiasOff {
    size_t ln1, attn, proj, ln2, fc, proj2;
};


struct mgpt_gpt {
    int L, nh, C, hs, block, max_rows;
    size_t n_params = 0;
    size_t off_wte = 0, off_wpe = 0, off_lnf = 0;
    std::vector<LayerOff> layers;
    float *params = nullptr;          // fp32 master copy, device
    std::vector<uint8_t> is_set;      // per parameter tensor
    // bias = True checkpoints: allocated (zeroed) by the first *.bias tensor mgpt_gpt_set_param sees; carried by the exact-fp32 kernels only
    float *bias = nullptr;            // [ln_f C | per layer: ln_1 C, c_attn 3C, attn c_proj C, ln_2 C, c_fc 4C, mlp c_proj C], device
    size_t off_lnf_b = 0;
    std::vector<BiasOff> bias_layers;
    std::vector<uint8_t> bias_set;    // per bias tensor: [ln_f | 6 per layer]
    bool has_bias = false;
    bool finalized = false;
    // fp32-path workspace
    float *x = nullptr, *xn = nullptr, *qkv = nullptr, *hbuf = nullptr, *logits_tmp = nullptr;
    // fast-path state (gpt_fast.hip)
    void *fast = nullptr;
    float *embed_table = nullptr;     // C = 256: [256 positions][67 tokens][C] = wpe + wte, the rows layer 0's attention block starts from (gpt_fast.hip)
    uint64_t generation = 1;          // bumped when weight planes / workspaces are freed or rebuilt (common.h: gpt_generation)
    // precision envelope of the split-fp16 mode (gpt.hip: envelope_*; include/mapf_gpt_amd.h: mgpt_gpt_envelope)
    float env_max_w = 0.f, env_max_rms = 0.f;   // over the 2-D matrices of the blocks, computed by mgpt_gpt_finalize
    float env_probe_err = -1.f;                 // max |f16x3 - f32| over the probe rows' logits, both call regimes (-1: not probed)
    float env_probe_err_small = -1.f, env_probe_err_large = -1.f;   // ... by regime: the kernels of calls <= / > kSmallRows rows
    float env_probe_tol = 0.f, env_probe_max_logit = 0.f;           // the bar it was held to, and max |logit| of the fp32 path
    int env_policy = 0;                         // MGPT_ENVELOPE_FALLBACK / _REFUSE / _IGNORE
    int env_state = 0;                          // 0 not decided, 1 inside, 2 outside
    bool env_logged = false;
    // training (train.hip): workspace of mgpt_gpt_train_alloc, NULL for a model that never trains
    void *train = nullptr;
    bool stale16 = false;                       // params changed in place (optimizer step): 16-bit planes and envelope rebuilt before the next 16-bit call
    // owners of the device memory above (device_mem.h); the precision modes and the training workspace own theirs (gpt_fast.hip, train.hip)
    mgpt::DeviceArena mem;                      // params, the fp32-path workspace, bias
    mgpt::DeviceArena embed_mem;                // embed_table
};


// outputs of a sequence forward (mgpt_gpt_forward_seq) for one chunk of rows: logits of every position [rows][T][67] or NULL; targets [rows][T]
// (-1 = ignored) with the per-row sum of the targeted positions' -log softmax and their count, or all three NULL
struct SeqOut {
    float *logits = nullptr;
    const int32_t *targets = nullptr;
    float *row_nll = nullptr;
    int32_t *row_count = nullptr;
};

// gpt_fast.hip: 16-bit-MFMA path (packed operand planes, own workspace)
int gpt_fast_finalize(mgpt_gpt *g);
void gpt_fast_destroy(mgpt_gpt *g);
// call_rows = rows of the whole C-ABI call this chunk belongs to: path choices that change the arithmetic (the head-parallel small-launch
// kernels) are made from it, so that every chunk of one call -- a ragged remainder included -- runs the same kernels.
// seq != NULL: the last layer runs at every position (the kernels of layers 0 .. L-2) and gpt_launch_head_seq replaces the head; d_logits unused
int gpt_fast_forward(mgpt_gpt *g, const uint8_t *d_tokens, int rows, float *d_logits, int precision, hipStream_t s, int call_rows,
                     const SeqOut *seq = nullptr);
int gpt_fast_debug_copy(mgpt_gpt *g, int precision, int which, void *d_out, int64_t nbytes, hipStream_t s);

// gpt.hip: reference state_dict key -> (tensor index, offset into params, element count); false for an unknown key
bool gpt_locate_param(const mgpt_gpt *g, const char *name, size_t *idx, size_t *off, size_t *count);
// gpt.hip: the parameters changed in place -- every precision serves the new weights: the fp32 kernels at once, the 16-bit planes, the layer-0
// tables and the envelope decision are rebuilt before the next 16-bit call; `generation` is bumped so that captured step graphs re-capture
void gpt_params_changed(mgpt_gpt *g);
// gpt.hip: the exact-fp32 forward kernels one by one (256-token rows; the forward of mgpt_gpt_forward_backward).  linear kind: 0 store,
// 1 add into out (the residual), 2 q|k|v scatter into head-major planes of M * C floats
int gpt_f32_embed(mgpt_gpt *g, const uint8_t *d_tokens, float *x, int64_t M, hipStream_t s);
int gpt_f32_layernorm(mgpt_gpt *g, const float *x, const float *w, float *y, int64_t n_tok, hipStream_t s);
int gpt_f32_linear(mgpt_gpt *g, int kind, const float *A, const float *W, float *out, int64_t M, int N, int K, hipStream_t s);
int gpt_f32_attention(mgpt_gpt *g, const float *qkv, float *y, int rows, hipStream_t s);
// train.hip: frees the training workspace (mgpt_gpt_destroy)
void gpt_train_destroy(mgpt_gpt *g);

// gpt.hip: final LayerNorm + tied lm_head on the last position of g->x (shared by both paths)
int gpt_launch_head(mgpt_gpt *g, int rows, float *d_logits, hipStream_t s);
int gpt_launch_head_at(mgpt_gpt *g, const float *xsrc, int64_t row_stride, int64_t row_offset, int rows, float *d_logits,
                       hipStream_t s);
// gpt.hip: ln_f + head + cross-entropy on EVERY position of rows x T tokens of x (tiled: fastk::xt_off layout), seqk::head_seq_kernel
int gpt_launch_head_seq(mgpt_gpt *g, const float *x, bool tiled, int rows, int T, const SeqOut &o, hipStream_t s);
