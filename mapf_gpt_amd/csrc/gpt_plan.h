// gpt_plan.h -- which kernels a chunk of the 16-bit forward runs, as host-only code: no runtime header, no pointer, so that the table
// of DESIGN.md section 3.2 compiles with any C++17 compiler and is checked cell by cell without a device (tests/host/plan_check.cpp).
//   mode_facts()  the one place that turns a shape into a family; called once when a precision mode is built (ModeState::facts)
//   make_plan()   the one place where the family, the precision mode and the row counts are looked at, once per chunk; where two
//                 conditions can hold at once, the order of the ?: chains is the precedence
// gpt_fast.hip holds the other halves: ModeBuilder fills the buffers a family's kernels need, Chunk launches what the plan names.
#pragma once
#include <algorithm>
#include <cstdint>

// calls of up to kSmallRows rows (one environment) run other kernels than larger ones (head-parallel attention, 32 x 32 x 16 MLP
// block, one-launch last layer).  For the C = 64 / 160 attention block: beyond ~164 rows of 5 heads the (row, head) workgroups need more
// rounds on 256 CUs than one workgroup per row takes (25 us against 80 us per workgroup, profiles/r02_cfg1_step_trace.txt)
constexpr int kSmallRows = 128;

namespace mgpt {
constexpr int kPlanT = 256;     // tokens per row

enum Family {               // fixed when the mode is built (mode_facts)
    FAM_REGISTER,           // C = 64 / 160, heads of 32: a layer is one attention-block kernel + one MLP-block kernel, q, k, v, y and the hidden stay on chip
    FAM_6M,                 // C = 256, 8 heads of 32: the same, with kernels of its own
    FAM_PACKED,             // any other C % 256 == 0 (85M): chain of packed-fragment GEMMs (gemm_pk) around attn16_kernel
    FAM_GENERIC             // everything else: gemm16 chain on row-major planes (C = 64 with one head of 64: its MLP block is still the fused kernel)
};
enum EmbedKind {            // where x = wte[token] + wpe[position] comes from
    EMBED_TABLE256,         // layer 0's attn256q_kernel reads the (position, token) table: x rows (EMB), or q | k | v themselves (TAB = 2, Plan::l0_qkv_table)
    EMBED_TABLE160,         // layer 0's attn160o_kernel<EMB> reads the table
    EMBED_ATTN_BLOCK,       // layer 0's attn_block_kernel<EMBED> gathers wte and wpe itself
    EMBED_TILED,            // embed_tiled_kernel (chunk-major x)
    EMBED_STATS             // embed_stats_kernel (row-major x + LayerNorm statistics)
};
enum AttnKind {             // the attention block of a full layer
    ATTN_160O,              // attn160o_kernel: persistent, whole block
    ATTN_BLOCK,             // attn_block_kernel: one workgroup per row, or per (row, head) in small calls (Plan::head_par)
    ATTN_256Q,              // attn256q_kernel: persistent, whole block
    ATTN_256_HEADS,         // attn256_kernel per (row, head) -> y planes -> packed out-projection
    ATTN_PACKED,            // (ln_pack) q|k and v^T gemm_pk, attn16_kernel, out-projection gemm_pk
    ATTN_GENERIC            // the same chain on gemm16
};
enum LastKind {             // the last layer, of which only token 255 of every row is needed (model.py:186)
    LAST_NONE,              // runs as a full layer: sequence forward (every position is needed), or FAM_GENERIC
    LAST_TAIL,              // small call: attention block, MLP block, ln_f and head in one attn_last1_kernel<.., 1, TAIL> launch; ends the chunk
    LAST_1,                 // attn_last1_kernel -> x_last, then the MLP block on the compact rows
    LAST_PACKED             // the packed chain with a compact tail: attn16 for query 255, gather_last, out-projection and MLP on rows_pad tokens
};
enum MlpKind { MLP_256P2, MLP_256P, MLP_256Q, MLP_160P, MLP_FUSED, MLP_FUSED16, MLP_PACKED, MLP_GENERIC };

// Everything about a built precision mode that dispatch depends on.  ModeBuilder allocates and packs by it, make_plan and Chunk launch by it.
struct ModeFacts {
    int C, L, nh, hs, max_rows;     // the model's shape and the context's row capacity
    int np, n_cu;                   // planes per operand (2: split fp16, 1: bf16); compute units of the model's device (grid of the persistent kernels)
    Family family;
    bool mlp_fused;                 // the MLP block is one kernel: FAM_REGISTER, FAM_6M, and C = 64 with one head of 64 (FAM_GENERIC)
    bool ln_fold;                   // LayerNorm folded into the packed GEMMs (GemmArgs): one-plane mode of FAM_PACKED unless MGPT_LN_FOLD=0
    bool l0_qkv_table;              // layer 0's q | k | v from a (position, token) table: FAM_6M with L > 1 unless MGPT_L0_TABLE=0
    // functions of the family
    bool x_tiled() const { return family != FAM_GENERIC; }                          // residual stream chunk-major (fastk::xt_off)
    bool qkv_on_chip() const { return family == FAM_REGISTER || family == FAM_6M; }   // no q|k, v^T planes in HBM: the attention kernels project
    bool pk_gemm() const { return family == FAM_PACKED || family == FAM_6M; }       // packed-fragment streams (6M: its small calls' out-projection)
    bool last1() const { return qkv_on_chip(); }                                    // fp32 last-layer weights of attn_last1_kernel
};

// want_l0_table, want_ln_fold: what MGPT_L0_TABLE / MGPT_LN_FOLD ask for (read once at build, gpt_fast.hip)
inline ModeFacts mode_facts(int C, int L, int nh, int hs, int max_rows, int np, int n_cu, bool want_l0_table, bool want_ln_fold)
{
    ModeFacts f = {C, L, nh, hs, max_rows, np, n_cu};
    // (C = 256: the fused kernels are the 6M shape's; any other C = 256 model takes the packed-fragment GEMM chain)
    f.family = (C == 256 && hs == 32 && nh == 8) ? FAM_6M : ((C == 160 || C == 64) && hs == 32) ? FAM_REGISTER
               : (C == 256 || C == 512 || C == 768 || C == 1024) ? FAM_PACKED : FAM_GENERIC;
    f.mlp_fused = f.family == FAM_6M || C == 160 || C == 64;
    // one-plane mode of the full chain: ln_pack_kernel, which re-reads every residual row to normalise it (8 % of an 85M step), runs once per forward, not twice per
    // layer.  (MGPT_LN_FOLD=0: the raw planes round x itself to bf16, which loses precision where a row's mean is many times its deviation)
    f.ln_fold = np == 1 && f.family == FAM_PACKED && want_ln_fold;
    f.l0_qkv_table = f.family == FAM_6M && L > 1 && want_l0_table;
    return f;
}

struct Plan {
    int rows, rows_pad;     // of the chunk; rounded up to 256 (compact last-layer buffers)
    int64_t M;              // tokens
    // a small call (one environment): its kernels spread few rows over the CUs.  Decided by the CALL's row count, not the chunk's: the remainder
    bool small;             // chunk of a large call stays on the large-call kernels
    bool big_call;          // the one-plane packed GEMMs run on the 16 x 16 x 32 MFMA (launch_gemm_pk)
    Family family;
    EmbedKind embed;
    bool l0_qkv_table;      // EMBED_TABLE256: layer 0's q | k | v from the mode's table (ModeFacts::l0_qkv_table)
    AttnKind attn;
    bool head_par;          // ATTN_BLOCK per (row, head): the heads' c_proj contributions go to head_parts and the MLP kernel folds them in
    int64_t part_stride;    // of head_parts
    LastKind last;
    bool last1_row_per_wg;  // LAST_1 with one row per workgroup instead of kLast1R (few rows on the 6M shape: so that they spread over the CUs)
    MlpKind mlp;
    int mlp160_tokens;      // MLP_160P: tokens per block (128: two waves per SIMD; 64, 32: so few tokens that larger blocks would leave CUs idle)
    int mlp_nw, mlp_nw_last;   // MLP_FUSED / MLP_FUSED16: waves per workgroup (32 tokens each) of a full layer and of the compact last layer
    bool half_qkv, half_proj, half_proj2;   // 128-row tiles in the packed GEMMs of small calls (q|k and v^T; out-projection and c_proj of full layers)
};

inline Plan make_plan(const ModeFacts &f, int rows, int call_rows, bool seq)
{
    Plan p = {};
    const int C = f.C, n_cu = f.n_cu;
    const bool reg = f.family == FAM_REGISTER, six = f.family == FAM_6M;
    p.rows = rows; p.rows_pad = ((rows + 255) / 256) * 256; p.M = (int64_t)rows * kPlanT;
    p.small = call_rows <= kSmallRows && rows <= kSmallRows;
    p.big_call = call_rows > kSmallRows;
    p.family = f.family;
    p.head_par = reg && p.small;
    p.part_stride = (int64_t)std::min(f.max_rows, kSmallRows) * kPlanT * C;       // (rows a small launch of this context can have)
    // the first attention block forms x = wte[token] + wpe[position] itself (no embedding kernel, no first read of x) ... unless the persistent block
    // kernel of the 2M shape serves the layer (profiles/r06_ab.txt visit B): embed_tiled_kernel + attn160o_kernel (0.6 + 4.5 ms per 16 384 rows) beat attn_block_kernel<EMBED> (5.8 ms)
    const bool persistent160 = reg && C == 160 && !p.head_par;
    const bool embed_fused = reg && f.L > 1 && !p.head_par && !persistent160;
    // ... and so do the persistent block kernels in a large call, from the (position, token) table (round 6)
    const bool embed256 = six && f.L > 1 && !p.small;
    const bool embed160 = persistent160 && f.L > 1;
    p.embed = embed256 ? EMBED_TABLE256 : embed160 ? EMBED_TABLE160 : embed_fused ? EMBED_ATTN_BLOCK : f.x_tiled() ? EMBED_TILED : EMBED_STATS;
    p.l0_qkv_table = f.l0_qkv_table;
    // 6M shape: attn256q_kernel does the out-projection and the residual add itself ... unless the call is small: then a row's eight heads
    // run on eight CUs at once (attn256_kernel, one workgroup per (row, head), y planes) and the packed GEMM projects them (round 5)
    const bool small256 = six && p.small;
    p.attn = persistent160 ? ATTN_160O : reg ? ATTN_BLOCK : six ? (small256 ? ATTN_256_HEADS : ATTN_256Q) : f.pk_gemm() ? ATTN_PACKED : ATTN_GENERIC;
    // last layer: only token 255 is needed downstream -> compact buffer, MLP and head on `rows` tokens.  The families with last1 weights
    // take LAST_TAIL in a small call and LAST_1 (without K and V: a launch that fills the chip) in a large one
    const bool short_last = f.x_tiled() && !seq;
    p.last = !short_last ? LAST_NONE : (p.head_par || small256) ? LAST_TAIL : f.last1() ? LAST_1 : LAST_PACKED;
    p.last1_row_per_wg = C == 256 && rows <= 2 * n_cu;
    // MLP block.  Small calls are not power-limited and keep the 32 x 32 x 16 kernels; large calls run the same block on v_mfma_f32_16x16x32
    // (mlp256q, mlp_fused16: 13-15 % more f16 flops per second at the power limit); the choice is a property of the call
    auto nw = [&](int64_t mlp_M) { return mlp_M >= (int64_t)256 * n_cu ? 8 : (mlp_M >= (int64_t)128 * n_cu ? 4 : 2); };
    p.mlp_nw = nw(p.M); p.mlp_nw_last = nw(p.rows_pad);
    p.mlp160_tokens = p.M <= (int64_t)32 * n_cu ? 32 : (p.M <= (int64_t)64 * n_cu ? 64 : 128);
    if (six) p.mlp = !small256 ? MLP_256Q : (2 * (int)(p.M / 128) <= n_cu ? MLP_256P2 : MLP_256P);
    else if (f.mlp_fused) p.mlp = (p.head_par && C == 160) ? MLP_160P : (p.head_par && C != 160) ? MLP_FUSED : MLP_FUSED16;
    else p.mlp = f.pk_gemm() ? MLP_PACKED : MLP_GENERIC;
    // the packed-GEMM chain (C = 768) in a small call: its residual GEMMs (N = 768: 3 column tiles) are 96 tiles of 256 rows for 32 rows -- 128-row
    // tiles put them on twice the CUs (same arithmetic per token: a wave's 64 x 128 sub-tile and its k order do not change).  One-plane mode: 32-row forward
    // 2.77 -> 2.49 ms (c_proj 70 -> 56 us, out-projection 30 -> 25, q|k + v^T 51 -> 47); in the split mode the 4-wave form has a 3-stage ring and loses (5.8 -> 6.4)
    const bool small_pk = f.np == 1 && f.family == FAM_PACKED && p.small;
    p.half_qkv = small_pk; p.half_proj = small256 || small_pk; p.half_proj2 = small_pk;
    return p;
}
}  // namespace mgpt
