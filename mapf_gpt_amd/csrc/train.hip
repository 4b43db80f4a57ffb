// train.hip -- training on the device (replaces train.py:324-331 with model.py:180-184 and :202-226): exact-fp32 or bf16 mixed-precision
// forward with saved activations, backward into one fp32 gradient buffer in the layout of mgpt_gpt::params, torch's clip_grad_norm_ and AdamW.
//
// A call (train_call: the checks and the chunk loop of both entry points) runs in chunks of the workspace's max_rows rows.  chunk_fwd_bwd is
// the one sequence of both precisions and both calls, its steps members of Chunk: embed, layer_forward per layer, head forward and loss, head
// backward, layer_backward per layer in reverse, embedding backward.  The bf16 path reaches the shared, fp32-sized workspace through typed
// views (bf16_layer, bf16_grads).  Dropout is a DropCfg of the chunk: every site asks drops(site) and regenerates its mask from drop(site,
// layer, tokens); no mask is stored.  with_attn_kernel turns the head size and attention dropout into the attention kernels' HS and DROP.
//
// mgpt_gpt_forward_backward_rows(_drop) is the micro-step of rows with one targeted position, token 255 (every row the dataset path makes):
// chunk_fwd_bwd runs the last layer, ln_f, the head and the cross-entropy on the compact matrix of the rows' last tokens (Compact).  Its
// normaliser is the call's row count, a host-side number: that path holds no stream synchronise, no blocking copy and no host read of device
// memory.
//
// The token-wise steps -- a residual branch's join and gradient, the MLP and out-projection backward, the bf16 MLP forward, LayerNorm
// backward, the head -- are written once per precision on a Tokens: all tokens of the chunk (Chunk::all) or the compact ones (Compact::tok),
// which draw the general call's dropout masks at token 255.  A layer's dense and compact bodies hold what differs: attention, c_attn, ln_1
// and, in fp32, the forward's linears.
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"
#include "gpt_ctx.h"
#include "gpt_kernels_train.h"
#include "gpt_kernels_train_bf16.h"

using namespace mgpt;

namespace {

constexpr int kT = 256;
constexpr int kV = MGPT_VOCAB;
constexpr int kSlabTokens = 256;       // tokens per weight-gradient slab (at most kMaxSlabs slabs): shorter fmaf chains, summed in order
constexpr int kMaxSlabs = 64;

// Workspace of one chunk of max_rows rows, M = max_rows * 256 tokens.  Saved per layer: x in, ln_1(x), q|k|v planes (3), y, x mid, ln_2(x),
// c_fc pre-activation (4): 12 C floats per token and layer, plus the final x and ln_f(x) (2 C) -- 12 L C + 2 C floats per token.  Backward
// scratch: dx, d ln, dy, dq|dk|dv (3), dh (4), gelu(a) (4), gain terms -- 14 C, plus logits and their gradient (2 * 67), the token's loss
// term (1) and the attention statistics (3 n_head).  In all (12 L + 16) C + 135 + 3 n_head floats per token, times 256 tokens of 4 bytes:
// 6M 30.1 MB per row (25.7 MB of it saved activations), 2M 7.0 MB, 85M 127.5 MB (114.8 MB).  Independent of max_rows: the weight-gradient
// slabs (at most 64 x 4 C^2 floats; beyond 128 C rows the bf16 path's LayerNorm-gain partials, 2 C floats per row, are larger) and the
// gradients and AdamW moments (3 x the parameters).
struct TrainState {
    int max_rows = 0;
    int64_t M = 0;
    float *grads = nullptr, *exp_avg = nullptr, *exp_avg_sq = nullptr, *steps = nullptr;    // [n_params] x 3, [n_tensors]
    std::vector<float *> X, XN1, QKV, Y, XM, XN2, A;
    float *XF = nullptr, *XNF = nullptr, *LG = nullptr, *DLG = nullptr, *NLL = nullptr;
    float *DX = nullptr, *DXN = nullptr, *DY = nullptr, *DQKV = nullptr, *DH = nullptr;
    // fp32 path only: gelu(a), the LayerNorm gain terms, the attention statistics (bf16 keeps gelu(a) in A[l], fuses the gain sums and keeps
    // its statistics in Y[l]: bf16_layer)
    float *HT = nullptr, *GP = nullptr, *AST = nullptr;
    float *part = nullptr;                  // weight-gradient / gain / embedding slabs
    size_t part_elems = 0;
    int32_t *cnt = nullptr;                 // [0] targeted positions of the call, [1] invalid-target flag
    int32_t *h_cnt = nullptr;               // pinned host copy
    double *loss_acc = nullptr;
    float *coef = nullptr;
    trk::Blk *blk = nullptr;
    int n_blk = 0;
    double *norm_part = nullptr;
    DeviceArena mem;                        // gradients, AdamW state and bookkeeping (h_cnt included): live as long as the workspace
    DeviceArena act_mem;                    // activations and backward scratch of max_rows rows: re-sized by mgpt_gpt_train_alloc
};

TrainState *ts(mgpt_gpt *g) { return static_cast<TrainState *>(g->train); }

void free_activations(TrainState *t)
{
    t->act_mem.release();
    t->X.clear(); t->XN1.clear(); t->QKV.clear(); t->Y.clear(); t->XM.clear(); t->XN2.clear(); t->A.clear();
    t->max_rows = 0;
    t->M = 0;
    t->part_elems = 0;
}

struct TensorInfo {
    size_t off, count;
    int decay;
};

// parameter tensors in the order of mgpt_gpt::params (= n_tensors order of gpt.hip): wte, wpe, ln_f, then per layer ln_1, c_attn, c_proj, ln_2,
// c_fc, mlp.c_proj.  Weight decay on the tensors of dim >= 2 (model.py:209-214)
std::vector<TensorInfo> tensor_table(const mgpt_gpt *g)
{
    const size_t C = g->C;
    std::vector<TensorInfo> t;
    t.push_back({g->off_wte, kV * C, 1});
    t.push_back({g->off_wpe, (size_t)g->block * C, 1});
    t.push_back({g->off_lnf, C, 0});
    for (const LayerOff &lo : g->layers) {
        t.push_back({lo.ln1, C, 0});
        t.push_back({lo.attn_w, 3 * C * C, 1});
        t.push_back({lo.proj_w, C * C, 1});
        t.push_back({lo.ln2, C, 0});
        t.push_back({lo.fc_w, 4 * C * C, 1});
        t.push_back({lo.proj2_w, 4 * C * C, 1});
    }
    return t;
}

// a failed step ends the sequence with its code
#define MGPT_TRY(call) do { const int rc__ = (call); if (rc__ != MGPT_OK) return rc__; } while (0)
// a launch and its MGPT_LAUNCH_CHECK
#define MGPT_LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); MGPT_LAUNCH_CHECK(); } while (0)

// weight-gradient, gain and embedding partials: slabs of tokens, `align`-token aligned (16: the fp32 kernels' k tile, 32: one bf16 MFMA's k)
int slabs_of(int64_t M) { return (int)std::min<int64_t>(kMaxSlabs, std::max<int64_t>(1, cdiv64(M, kSlabTokens))); }
int slab_tokens(int64_t M, int align) { return (int)((cdiv64(M, slabs_of(M)) + align - 1) / align * align); }

unsigned grid_1d(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n, 256), 8192)); }

// ----- the bf16 path's views of the workspace -----
// Both precisions share one workspace, sized for fp32 (TrainState).  A bf16 chunk of M tokens (M <= t->M) keeps its 16-bit tensors at the
// start of the fp32 buffers of the same role:
//   QKV[l] (3 M C floats)  the bf16 q | k | v planes, M C elements each;
//   Y[l]   (M C floats)    bf16 y, M C elements = M C / 2 floats, then the softmax statistics, 2 n_head floats per token.  They fit
//                          because 2 n_head <= C / 2 (any head size >= 4);
//   A[l]   (4 M C floats)  bf16 a, then bf16 gelu(a), 4 M C elements each: two bf16 per float, the whole buffer;
//   DY, DH (M C, 4 M C)    the bf16 gradients of y and of a, the first half of each.
// mgpt_gpt_train_alloc checks the two claims once; no layer body casts or offsets a buffer itself.
struct Bf16Layer { uint16_t *qkv, *y; float *stats; uint16_t *a, *h; };
struct Bf16Grads { uint16_t *dy, *da; };

Bf16Layer bf16_layer(const TrainState *t, int l, int64_t M, int C)
{
    uint16_t *y = reinterpret_cast<uint16_t *>(t->Y[l]), *a = reinterpret_cast<uint16_t *>(t->A[l]);
    return {reinterpret_cast<uint16_t *>(t->QKV[l]), y, reinterpret_cast<float *>(y + M * C), a, a + 4 * M * C};
}

Bf16Grads bf16_grads(const TrainState *t) { return {reinterpret_cast<uint16_t *>(t->DY), reinterpret_cast<uint16_t *>(t->DH)}; }

// ----- the compact matrix of the last-position micro-step -----
// The tokens a token-wise step runs over: all M tokens of the chunk (Chunk::all), or the mc compact tokens (Compact::tok).  With them their
// gradient scratch (d x, d ln, the gain terms), the slot m s d x is written to before a masked branch's c_proj (drop_dx), and the slot a
// masked fp32 branch's output passes through before it joins the residual (drop_out).  last: the tokens are token 255 of each row, so
// their dropout masks lie 256 C elements apart from token 255 of the chunk's first row on (Chunk::drop), and the elementwise kernels and
// the epilogue that draw them are the _last ones.
struct Tokens { int64_t m; float *dx, *dxn, *gp, *drop_dx, *drop_out; bool last; };

// A chunk of n rows keeps mc compact tokens, one per row (token 255), in the slots its last layer l = L - 1 does not fill.  mc = n in fp32
// (gemm_tr_kernel checks every index); in bf16 n rounded up to 32, the MFMA GEMMs' k step, the padding rows zero (gather_last_kernel,
// ce_rows_kernel), and zero rows stay zero through LayerNorm, the linears, GELU and their backward.  A slot of M C = 256 n C floats holds
// eight compact matrices of mc C floats (mc <= 32 n): sub(slot, i).
//   QKV[l] plane 0  q (the k and v planes are the general path's, filled for all tokens)
//   Y[l]            y | ln_1(x) of token 255 | x of token 255
//   XM[l], XN2[l], A[l], XF, XNF, LG, DLG, NLL, HT, DH   their roles, mc tokens (bf16: bf16_layer(t, l, mc, C)'s a and h, bf16_grads' da)
//   AST             the softmax statistics (m, 1 / l) per (row, head), in both precisions
//   DY              d y | d x | d ln | gain terms | d q | d ln_1 of token 255 | under dropout: a branch's output before its mask joins
//                   (forward, fp32), then m s d x, the gradient that enters a branch's c_proj (backward)
struct Compact {
    int n, mc;
    float *q, *y, *xn1, *x, *dy, *dq, *dxn1;
    Tokens tok;
};

Compact compact_of(const TrainState *t, int l, int n, bool bf16, int C)
{
    const int mc = bf16 ? (n + 31) / 32 * 32 : n;
    auto sub = [&](float *slot, int i) { return slot + (size_t)i * mc * C; };
    return {n, mc, t->QKV[l], t->Y[l], sub(t->Y[l], 1), sub(t->Y[l], 2), t->DY, sub(t->DY, 4), sub(t->DY, 5),
            {(int64_t)mc, sub(t->DY, 1), sub(t->DY, 2), sub(t->DY, 3), sub(t->DY, 6), sub(t->DY, 6), true}};
}

// ----- epilogue arguments of gemm_bf16_kernel, one constructor per kind (the fields a kind does not read stay zero) -----
tbk::Epi epi_f32(float *out, int64_t ldc) { tbk::Epi e; e.f32 = out; e.ldc = ldc; return e; }                              // E_F32, E_PART
tbk::Epi epi_resid(float *out, const float *res, int64_t ldc) { tbk::Epi e = epi_f32(out, ldc); e.res = res; return e; }    // E_RESID
tbk::Epi epi_b16(uint16_t *out, int64_t ldc) { tbk::Epi e; e.b16 = out; e.ldc = ldc; return e; }                            // E_B16
tbk::Epi epi_fc(uint16_t *a, uint16_t *h, int64_t ldc) { tbk::Epi e = epi_b16(a, ldc); e.b16b = h; return e; }              // E_FC
tbk::Epi epi_gelu_bwd(uint16_t *da, const uint16_t *a, int64_t ldc) { tbk::Epi e = epi_b16(da, ldc); e.aux = a; return e; }  // E_GELU_BWD
tbk::Epi epi_qkv(uint16_t *planes, int C, int hs, int n_head, int64_t plane)                                                // E_QKV
{
    tbk::Epi e;
    e.b16 = planes; e.C = C; e.hs = hs; e.n_head = n_head; e.plane = plane;
    return e;
}

// the attention kernels' dynamic LDS exceeds the default limit: raised once per workspace (mgpt_gpt_train_alloc), for the model's head size
template <int HS>
int raise_attn_lds()
{
    const std::pair<const void *, size_t> kernels[] = {
        {reinterpret_cast<const void *>(&trk::attn_bwd_q_kernel<HS>), trk::attn_bwd_q_lds<HS>()},
        {reinterpret_cast<const void *>(&trk::attn_bwd_kv_kernel<HS, 0>), trk::attn_bwd_kv_lds<HS>()},
        {reinterpret_cast<const void *>(&trk::attn_bwd_kv_kernel<HS, 1>), trk::attn_bwd_kv_lds<HS>()},
        {reinterpret_cast<const void *>(&tbk::attn_fwd_bf16_kernel<HS>), tbk::attn_fwd_lds<HS>()},
        {reinterpret_cast<const void *>(&tbk::attn_bwd_bf16_kernel<HS>), tbk::attn_bwd_lds<HS>()},
        {reinterpret_cast<const void *>(&trk::attn_bwd_q_kernel<HS, true>), trk::attn_bwd_q_lds<HS>()},
        {reinterpret_cast<const void *>(&trk::attn_bwd_kv_kernel<HS, 0, true>), trk::attn_bwd_kv_lds<HS>()},
        {reinterpret_cast<const void *>(&trk::attn_bwd_kv_kernel<HS, 1, true>), trk::attn_bwd_kv_lds<HS>()},
        {reinterpret_cast<const void *>(&tbk::attn_fwd_bf16_kernel<HS, true>), tbk::attn_fwd_lds<HS>()},
        {reinterpret_cast<const void *>(&tbk::attn_bwd_bf16_kernel<HS, true>), tbk::attn_bwd_lds<HS>()}};
    for (const auto &k : kernels) MGPT_HIP(set_max_lds(k.first, (int)k.second));
    return MGPT_OK;
}

// Dropout of one chunk (mgpt_gpt_forward_backward_drop): thr = 0 or sites = 0 is no dropout, and then every launch is the one of
// mgpt_gpt_forward_backward_prec.  first_row = row0 + the chunk's first row within the call: the masks are keyed by the row of the call.
enum { SITE_EMBED = 0, SITE_ATTN = 1, SITE_ATTN_PROJ = 2, SITE_MLP_PROJ = 3 };
struct DropCfg {
    uint32_t thr = 0;
    float scale = 1.f;
    uint64_t seed = 0, step = 0, first_row = 0;
    int sites = 0;
};

// One chunk of rows of a call: what its launches share, and the launches (chunk_fwd_bwd is the sequence).  The layer's steps and
// ln_backward have a body per precision; the head and the embedding run the fp32 kernels in both.  call_rows > 0: the rows call, tg its
// labels, one per row, and call_rows the row count of the whole call.
// bf16 (MGPT_PREC_BF16) is train.py's autocast regime on bf16 MFMAs (gpt_kernels_train_bf16.h).  Rounded to bf16, as autocast holds them: the operands of the
// block linears, q, k, v, attention's output and its gradient, P and dS, the linears' outputs and GELU's, the gradients of the MLP hidden
// tensors.  fp32: the embedding sum, the residual stream and its gradient, LayerNorm, softmax statistics, the head, cross-entropy and every
// accumulator.
struct Chunk {
    mgpt_gpt *g;
    TrainState *t;
    const uint8_t *tok;
    const int32_t *tg;
    int rows, call_rows;
    float loss_scale;
    bool bf16;
    hipStream_t s;
    DropCfg dc;
    const int C = g->C, L = g->L;
    const int64_t M = (int64_t)rows * kT;
    const float *P = g->params;
    float *G = t->grads;
    const float scale = 1.0f / sqrtf((float)g->hs);

    float *x_out(int l) const { return l + 1 < L ? t->X[l + 1] : t->XF; }

    // all tokens of the chunk: the masked branch gradient goes to DXN (free at both points of layer_backward), a masked fp32 branch output
    // through DY (free during the forward)
    Tokens all() const { return {M, t->DX, t->DXN, t->GP, t->DXN, t->DY, false}; }
    // the last layer's compact tokens (the rows call)
    Compact compact() const { return compact_of(t, L - 1, rows, bf16, C); }

    // ----- dropout: is the site on, its mask stream for this chunk, and the elementwise launches over the tokens' m x C elements -----
    bool drops(int site) const { return dc.thr > 0 && ((dc.sites >> site) & 1); }
    trk::Drop drop(int site, int layer) const
    {
        trk::Drop d;
        d.key = trk::drop_key(dc.seed, dc.step, site, layer);
        d.base = dc.first_row * (site == SITE_ATTN ? (uint64_t)g->nh * kT * kT : (uint64_t)kT * C);
        d.thr = dc.thr;
        d.scale = dc.scale;
        return d;
    }
    // ... of sites 0, 2 and 3 over `tk`: the compact tokens' base is token 255 of the chunk's first row
    trk::Drop drop(int site, int layer, const Tokens &tk) const
    {
        trk::Drop d = drop(site, layer);
        if (tk.last) d.base += (uint64_t)(kT - 1) * C;
        return d;
    }
    // out = m s in (in rounded to bf16 first in the bf16 path's backward: the gradient of a bf16 branch output)
    int drop_scale(int site, int layer, const Tokens &tk, const float *in, float *out, bool round = false)
    {
        const int64_t n4 = tk.m * C / 4;
        const dim3 grid(grid_1d(n4));
        const trk::Drop d = drop(site, layer, tk);
        if (tk.last) {
            if (round) MGPT_LAUNCH(trk::drop_scale_last_kernel<true>, grid, dim3(256), 0, s, in, out, (int)tk.m, C, d);
            else MGPT_LAUNCH(trk::drop_scale_last_kernel<false>, grid, dim3(256), 0, s, in, out, (int)tk.m, C, d);
        } else if (round) MGPT_LAUNCH(trk::drop_scale_kernel<true>, grid, dim3(256), 0, s, in, out, n4, d);
        else MGPT_LAUNCH(trk::drop_scale_kernel<false>, grid, dim3(256), 0, s, in, out, n4, d);
        return MGPT_OK;
    }
    // the gradient that enters a residual branch's c_proj: the tokens' dx, or m s dx in their drop_dx (zero padding rows stay zero)
    int branch_grad(int site, int layer, const Tokens &tk, const float **db)
    {
        *db = tk.dx;
        if (!drops(site)) return MGPT_OK;
        *db = tk.drop_dx;
        return drop_scale(site, layer, tk, tk.dx, tk.drop_dx, bf16);
    }
    // fp32 path: out = x + m s (A W^T), the masked branch's output through the tokens' drop_out.  All tokens: the inference linear, which
    // accumulates onto a copy of x; the compact ones: gemm_tr_kernel, which checks every index
    int branch_forward_f32(int site, int layer, const Tokens &tk, const float *A, const float *W, int K, const float *x, float *out)
    {
        const int64_t n4 = tk.m * C / 4;
        if (tk.last) {
            if (!drops(site)) return tr_gemm<true, false, trk::OUT_RESID>(A, K, W, K, out, C, tk.m, C, K, x);
            MGPT_TRY((tr_gemm<true, false, trk::OUT_STORE>(A, K, W, K, tk.drop_out, C, tk.m, C, K)));
            MGPT_LAUNCH(trk::drop_resid_last_kernel, dim3(grid_1d(n4)), dim3(256), 0, s, x, (const float *)tk.drop_out, out, (int)tk.m, C, drop(site, layer, tk));
            return MGPT_OK;
        }
        if (!drops(site)) {
            MGPT_HIP(hipMemcpyAsync(out, x, (size_t)tk.m * C * sizeof(float), hipMemcpyDeviceToDevice, s));
            return gpt_f32_linear(g, 1, A, W, out, tk.m, C, K, s);
        }
        MGPT_TRY(gpt_f32_linear(g, 0, A, W, tk.drop_out, tk.m, C, K, s));
        MGPT_LAUNCH(trk::drop_resid_kernel, dim3(grid_1d(n4)), dim3(256), 0, s, x, (const float *)tk.drop_out, out, n4, drop(site, layer, tk));
        return MGPT_OK;
    }
    // bf16 path: out = x + bf16(m s bf16(A W^T)) in the GEMM's epilogue (the compact tokens' padding rows stay zero: x and A are zero there)
    template <typename TA>
    int branch_forward_bf16(int site, int layer, const Tokens &tk, const TA *A, const float *W, int K, const float *x, float *out)
    {
        tbk::Epi e = epi_resid(out, x, C);
        if (!drops(site)) return bf_gemm<TA, true, float, true, tbk::E_RESID>(A, K, W, K, tk.m, C, K, e);
        e.drop = drop(site, layer, tk);
        if (!tk.last) return bf_gemm<TA, true, float, true, tbk::E_RESID_DROP>(A, K, W, K, tk.m, C, K, e);
        e.plane = (int64_t)kT * C;
        return bf_gemm<TA, true, float, true, tbk::E_RESID_DROP_LAST>(A, K, W, K, tk.m, C, K, e);
    }

    // out[m][N] (op)= A'(m x K) @ B'(K x N), fp32 on the VALU; slabs > 1: one partial per kps of K
    template <bool A_KC, bool B_NC, int OUT>
    int tr_gemm(const float *A, int64_t lda, const float *B, int64_t ldb, float *out, int64_t ldc, int64_t m, int N, int K, const float *aux = nullptr,
                int slabs = 1, int kps = 0)
    {
        const dim3 grid((unsigned)cdiv(N, 64), (unsigned)cdiv64(m, 64), (unsigned)slabs);
        MGPT_LAUNCH((trk::gemm_tr_kernel<A_KC, B_NC, OUT>), grid, dim3(256), 0, s, A, lda, B, ldb, out, ldc, (int)m, N, K, slabs == 1 ? K : kps, aux);
        return MGPT_OK;
    }

    // ... on bf16 MFMAs, the output named by the epilogue
    template <typename TA, bool A_KC, typename TB, bool B_KC, int EPI>
    int bf_gemm(const TA *A, int64_t lda, const TB *B, int64_t ldb, int64_t m, int N, int K, const tbk::Epi &ep, int slabs = 1, int kps = 0)
    {
        if (slabs == 1) kps = K;
        MGPT_REQUIRE(m % 16 == 0 && N % 16 == 0 && K % 32 == 0 && kps % 32 == 0 && m <= INT32_MAX, MGPT_ERR_UNSUPPORTED,
                     "bf16 gemm shape M=%lld N=%d K=%d (slab %d)", (long long)m, N, K, kps);
        const dim3 grid((unsigned)cdiv(N, tbk::BN), (unsigned)cdiv64(m, tbk::BM), (unsigned)slabs);
        MGPT_LAUNCH((tbk::gemm_bf16_kernel<TA, A_KC, TB, B_KC, EPI>), grid, dim3(256), 0, s, A, lda, B, ldb, (int)m, N, K, kps, ep);
        return MGPT_OK;
    }

    // ----- sums over m tokens by slabs: partials(S, kps) launches S partial sums of kps tokens each into t->part [S][n], which are added to
    // out[n] in order -----
    template <class Launch>
    int slab_sum(float *out, int64_t n, int align, int64_t m, Launch partials)
    {
        const int S = slabs_of(m), kps = slab_tokens(m, align);
        MGPT_REQUIRE((size_t)S * n <= t->part_elems, MGPT_ERR_ARG, "weight-gradient slabs exceed the workspace");
        MGPT_TRY(partials(S, kps));
        MGPT_LAUNCH(trk::slab_reduce_kernel, dim3(grid_1d(n)), dim3(256), 0, s, t->part, S, n, out);
        return MGPT_OK;
    }

    // weight gradients: dW[Nout][Kin] += dY^T @ X over m tokens, dY [m][Nout] with row pitch ldy, X [m][Kin]; fp32 on the VALU, or bf16
    // MFMAs (32-token aligned slabs)
    int weight_grad(const float *dY, int64_t ldy, const float *X, float *dW, int Nout, int Kin, int64_t m)
    {
        return slab_sum(dW, (int64_t)Nout * Kin, 16, m, [&](int S, int kps) -> int {
            return tr_gemm<false, true, trk::OUT_PART>(dY, ldy, X, Kin, t->part, Kin, Nout, Kin, (int)m, nullptr, S, kps);
        });
    }

    template <typename TY, typename TX>
    int weight_grad_bf16(const TY *dY, int64_t ldy, const TX *X, float *dW, int Nout, int Kin, int64_t m)
    {
        return slab_sum(dW, (int64_t)Nout * Kin, 32, m, [&](int S, int kps) -> int {
            return bf_gemm<TY, false, TX, false, tbk::E_PART>(dY, ldy, X, Kin, Nout, Kin, (int)m, epi_f32(t->part, Kin), S, kps);
        });
    }

    // ----- LayerNorm backward over `sp`: dx (+)= d x from dxn, the gain's gradient gw += sum over the tokens of dxn * xhat -----
    template <bool ADD>
    int ln_backward_f32(const float *x, const float *w, float *gw, const Tokens &sp)
    {
        MGPT_LAUNCH((trk::ln_bwd_kernel<ADD>), dim3((unsigned)cdiv64(sp.m, 4)), dim3(256), 0, s, x, w, (const float *)sp.dxn, sp.dx, sp.gp, sp.m, C);
        return slab_sum(gw, C, 16, sp.m, [&](int S, int kps) -> int {
            MGPT_LAUNCH(trk::colsum_part_kernel, dim3((unsigned)cdiv(C, 256), (unsigned)S), dim3(256), 0, s, (const float *)sp.gp, sp.m, C, kps, t->part);
            return MGPT_OK;
        });
    }

    // ... with the gain's column sums fused: one partial per 128 tokens, summed in order
    template <bool ADD>
    int ln_backward_bf16(const float *x, const float *w, float *gw, const Tokens &sp)
    {
        const int64_t n_part = cdiv64(sp.m, tbk::kLnTok);
        MGPT_REQUIRE(C <= 64 * tbk::kLnMaxJ && (size_t)(n_part * C) <= t->part_elems, MGPT_ERR_UNSUPPORTED, "LayerNorm backward: C=%d, %lld tokens", C, (long long)sp.m);
        MGPT_LAUNCH((tbk::ln_bwd_gain_kernel<ADD>), dim3((unsigned)n_part), dim3(256), 0, s, x, w, (const float *)sp.dxn, sp.dx, t->part, sp.m, C);
        MGPT_LAUNCH(tbk::colsum_reduce_kernel, dim3((unsigned)cdiv(C, 64)), dim3(1024), 0, s, t->part, (int)n_part, C, gw);
        return MGPT_OK;
    }

    template <bool ADD>
    int ln_backward(const float *x, size_t gain, const Tokens &sp)
    {
        return bf16 ? ln_backward_bf16<ADD>(x, P + gain, G + gain, sp) : ln_backward_f32<ADD>(x, P + gain, G + gain, sp);
    }

    // ----- attention, one workgroup per (row, head) -----
    // The model's head size and whether site 1 drops, as the kernels' template arguments: launch(hs, dropped, d), hs and dropped
    // std::integral_constants of HS and DROP, d layer l's mask stream -- trk::Drop() for a DROP = false instance
    template <class Launch>
    int with_attn_kernel(int l, Launch launch)
    {
        using H32 = std::integral_constant<int, 32>;
        using H64 = std::integral_constant<int, 64>;
        if (!drops(SITE_ATTN)) return g->hs == 32 ? launch(H32(), std::false_type(), trk::Drop()) : launch(H64(), std::false_type(), trk::Drop());
        const trk::Drop d = drop(SITE_ATTN, l);
        return g->hs == 32 ? launch(H32(), std::true_type(), d) : launch(H64(), std::true_type(), d);
    }

    // fp32 forward: the inference kernel, or the training instance that masks P
    int attn_forward_f32(int l)
    {
        if (!drops(SITE_ATTN)) return gpt_f32_attention(g, t->QKV[l], t->Y[l], rows, s);
        return with_attn_kernel(l, [&](auto hs, auto, const trk::Drop &d) -> int {
            MGPT_LAUNCH(trk::attn_fwd_drop_kernel<decltype(hs)::value>, dim3((unsigned)(rows * g->nh)), dim3(256), 0, s, (const float *)t->QKV[l], M * C, t->Y[l],
                        g->nh, scale, d);
            return MGPT_OK;
        });
    }

    // fp32 backward: dq | dk | dv of DY into DQKV
    int attn_backward_f32(int l, const float *qkv, const float *y)
    {
        return with_attn_kernel(l, [&](auto hs, auto dropped, const trk::Drop &d) -> int {
            constexpr int HS = decltype(hs)::value;
            constexpr bool DROP = decltype(dropped)::value;
            const dim3 grid((unsigned)(rows * g->nh));
            const int64_t plane = M * C;
            MGPT_LAUNCH((trk::attn_bwd_q_kernel<HS, DROP>), grid, dim3(256), trk::attn_bwd_q_lds<HS>(), s, qkv, plane, y, t->DY, t->DQKV, t->AST, g->nh, scale, d);
            MGPT_LAUNCH((trk::attn_bwd_kv_kernel<HS, 0, DROP>), grid, dim3(256), trk::attn_bwd_kv_lds<HS>(), s, qkv, plane, t->DY, t->DQKV, t->AST, g->nh, scale, d);
            MGPT_LAUNCH((trk::attn_bwd_kv_kernel<HS, 1, DROP>), grid, dim3(256), trk::attn_bwd_kv_lds<HS>(), s, qkv, plane, t->DY, t->DQKV, t->AST, g->nh, scale, d);
            return MGPT_OK;
        });
    }

    // bf16 MFMAs: forward (y bf16, statistics fp32) and backward (dq | dk | dv fp32 into DQKV)
    int attn_forward_bf16(int l, const Bf16Layer &v)
    {
        return with_attn_kernel(l, [&](auto hs, auto dropped, const trk::Drop &d) -> int {
            constexpr int HS = decltype(hs)::value;
            MGPT_LAUNCH((tbk::attn_fwd_bf16_kernel<HS, decltype(dropped)::value>), dim3((unsigned)(rows * g->nh)), dim3(256), tbk::attn_fwd_lds<HS>(), s, v.qkv, M * C,
                        v.y, v.stats, g->nh, scale, d);
            return MGPT_OK;
        });
    }

    int attn_backward_bf16(int l, const Bf16Layer &v, const uint16_t *dy)
    {
        return with_attn_kernel(l, [&](auto hs, auto dropped, const trk::Drop &d) -> int {
            constexpr int HS = decltype(hs)::value;
            MGPT_LAUNCH((tbk::attn_bwd_bf16_kernel<HS, decltype(dropped)::value>), dim3((unsigned)(rows * g->nh)), dim3(512), tbk::attn_bwd_lds<HS>(), s, v.qkv, M * C,
                        v.y, dy, v.stats, t->DQKV, g->nh, scale, d);
            return MGPT_OK;
        });
    }

    // query 255 of each row against the row's k and v planes, TQ float or bf16 bits: y and dq compact, dk | dv dense into DQKV.  The
    // kernels write the rows' tokens only: the padding rows of their compact outputs are zeroed (stream-ordered)
    int zero_pad(void *buf, size_t elem, const Compact &k)
    {
        if (k.mc > k.n) MGPT_HIP(hipMemsetAsync(static_cast<char *>(buf) + (size_t)k.n * C * elem, 0, (size_t)(k.mc - k.n) * C * elem, s));
        return MGPT_OK;
    }
    template <typename TQ>
    int attn_last_forward(const Compact &k, const TQ *q, const TQ *kp, const TQ *vp, TQ *y)
    {
        MGPT_TRY((with_attn_kernel(L - 1, [&](auto hs, auto dropped, const trk::Drop &d) -> int {
            MGPT_LAUNCH((trk::attn_last_fwd_kernel<decltype(hs)::value, TQ, decltype(dropped)::value>), dim3((unsigned)(k.n * g->nh)), dim3(256), 0, s, q, kp, vp, y,
                        t->AST, g->nh, scale, d);
            return MGPT_OK;
        })));
        return zero_pad(y, sizeof(TQ), k);
    }
    template <typename TQ>
    int attn_last_backward(const Compact &k, const TQ *q, const TQ *kp, const TQ *vp, const TQ *y, const TQ *dy)
    {
        MGPT_TRY((with_attn_kernel(L - 1, [&](auto hs, auto dropped, const trk::Drop &d) -> int {
            MGPT_LAUNCH((trk::attn_last_bwd_kernel<decltype(hs)::value, TQ, decltype(dropped)::value>), dim3((unsigned)(k.n * g->nh)), dim3(256), 0, s, q, kp, vp, y,
                        dy, (const float *)t->AST, t->DQKV, k.dq, g->nh, scale, d);
            return MGPT_OK;
        })));
        return zero_pad(k.dq, sizeof(float), k);
    }

    // ----- the steps of a layer that are the same launches over all tokens and over the compact ones -----
    // fp32: HT = gelu(a)
    int gelu(int l, const Tokens &tk)
    {
        MGPT_LAUNCH(trk::gelu_kernel, dim3(grid_1d(4 * tk.m * C)), dim3(256), 0, s, t->A[l], t->HT, 4 * tk.m * C);
        return MGPT_OK;
    }

    // bf16 MLP half (model.py:85-88,103): xo = xm + dropout(c_proj(gelu(c_fc(ln_2(xm))))), a and gelu(a) kept
    int mlp_forward_bf16(int l, const Tokens &tk, const float *xm, float *xo)
    {
        const LayerOff &lo = g->layers[l];
        const Bf16Layer v = bf16_layer(t, l, tk.m, C);
        MGPT_TRY(gpt_f32_layernorm(g, xm, P + lo.ln2, t->XN2[l], tk.m, s));
        MGPT_TRY((bf_gemm<float, true, float, true, tbk::E_FC>(t->XN2[l], C, P + lo.fc_w, C, tk.m, 4 * C, C, epi_fc(v.a, v.h, 4 * C))));
        return branch_forward_bf16(SITE_MLP_PROJ, l, tk, v.h, P + lo.proj2_w, 4 * C, xm, xo);
    }

    // MLP backward (model.py:85-88,103): the tokens' dx = d x_out becomes d x_mid; db = the gradient of c_proj's output (m s dx under dropout).
    // fp32: HT = gelu(a) of these tokens, recomputed first where `regelu`
    int mlp_backward_f32(int l, const Tokens &tk, bool regelu)
    {
        const LayerOff &lo = g->layers[l];
        const float *db;
        MGPT_TRY(branch_grad(SITE_MLP_PROJ, l, tk, &db));
        MGPT_TRY((tr_gemm<true, true, trk::OUT_GELU_BWD>(db, C, P + lo.proj2_w, 4 * C, t->DH, 4 * C, tk.m, 4 * C, C, t->A[l])));
        if (regelu) MGPT_TRY(gelu(l, tk));
        MGPT_TRY(weight_grad(db, C, t->HT, G + lo.proj2_w, C, 4 * C, tk.m));
        MGPT_TRY((tr_gemm<true, true, trk::OUT_STORE>(t->DH, 4 * C, P + lo.fc_w, C, tk.dxn, C, tk.m, C, 4 * C)));
        MGPT_TRY(weight_grad(t->DH, 4 * C, t->XN2[l], G + lo.fc_w, 4 * C, C, tk.m));
        return ln_backward<true>(t->XM[l], lo.ln2, tk);
    }
    // bf16: dx's bf16 rounding is the gradient of the bf16 c_proj output (under dropout db = m s bf16(dx), rounded as it is staged)
    int mlp_backward_bf16(int l, const Tokens &tk)
    {
        const LayerOff &lo = g->layers[l];
        const Bf16Layer v = bf16_layer(t, l, tk.m, C);
        const Bf16Grads d = bf16_grads(t);
        const float *db;
        MGPT_TRY(branch_grad(SITE_MLP_PROJ, l, tk, &db));
        MGPT_TRY((bf_gemm<float, true, float, false, tbk::E_GELU_BWD>(db, C, P + lo.proj2_w, 4 * C, tk.m, 4 * C, C, epi_gelu_bwd(d.da, v.a, 4 * C))));
        MGPT_TRY(weight_grad_bf16(db, C, v.h, G + lo.proj2_w, C, 4 * C, tk.m));
        MGPT_TRY((bf_gemm<uint16_t, true, float, false, tbk::E_F32>(d.da, 4 * C, P + lo.fc_w, C, tk.m, C, 4 * C, epi_f32(tk.dxn, C))));
        MGPT_TRY(weight_grad_bf16(d.da, 4 * C, t->XN2[l], G + lo.fc_w, 4 * C, C, tk.m));
        return ln_backward<true>(t->XM[l], lo.ln2, tk);
    }

    // attention's out-projection backward (model.py:71,102): the tokens' dx = d x_mid; dy = d y, c_proj's weight gradient from y
    int proj_backward_f32(int l, const Tokens &tk, const float *y, float *dy)
    {
        const LayerOff &lo = g->layers[l];
        const float *db;
        MGPT_TRY(branch_grad(SITE_ATTN_PROJ, l, tk, &db));
        MGPT_TRY((tr_gemm<true, true, trk::OUT_STORE>(db, C, P + lo.proj_w, C, dy, C, tk.m, C, C)));
        return weight_grad(db, C, y, G + lo.proj_w, C, C, tk.m);
    }
    // bf16: d y = bf16(db W_proj), the gradient of the bf16 attention output
    int proj_backward_bf16(int l, const Tokens &tk, const uint16_t *y, uint16_t *dy)
    {
        const LayerOff &lo = g->layers[l];
        const float *db;
        MGPT_TRY(branch_grad(SITE_ATTN_PROJ, l, tk, &db));
        MGPT_TRY((bf_gemm<float, true, float, false, tbk::E_B16>(db, C, P + lo.proj_w, C, tk.m, C, C, epi_b16(dy, C))));
        return weight_grad_bf16(db, C, y, G + lo.proj_w, C, C, tk.m);
    }

    // ----- a layer on all tokens -----
    // fp32 forward: the inference kernels
    int layer_forward_f32(int l)
    {
        const LayerOff &lo = g->layers[l];
        const Tokens tk = all();
        float *x = t->X[l], *xm = t->XM[l], *xo = x_out(l);
        MGPT_TRY(gpt_f32_layernorm(g, x, P + lo.ln1, t->XN1[l], M, s));
        MGPT_TRY(gpt_f32_linear(g, 2, t->XN1[l], P + lo.attn_w, t->QKV[l], M, 3 * C, C, s));
        MGPT_TRY(attn_forward_f32(l));
        MGPT_TRY(branch_forward_f32(SITE_ATTN_PROJ, l, tk, t->Y[l], P + lo.proj_w, C, x, xm));
        MGPT_TRY(gpt_f32_layernorm(g, xm, P + lo.ln2, t->XN2[l], M, s));
        MGPT_TRY(gpt_f32_linear(g, 0, t->XN2[l], P + lo.fc_w, t->A[l], M, 4 * C, C, s));
        MGPT_TRY(gelu(l, tk));
        return branch_forward_f32(SITE_MLP_PROJ, l, tk, t->HT, P + lo.proj2_w, 4 * C, xm, xo);
    }

    int layer_forward_bf16(int l)
    {
        const LayerOff &lo = g->layers[l];
        const Bf16Layer v = bf16_layer(t, l, M, C);
        float *x = t->X[l], *xm = t->XM[l];
        MGPT_TRY(gpt_f32_layernorm(g, x, P + lo.ln1, t->XN1[l], M, s));
        MGPT_TRY((bf_gemm<float, true, float, true, tbk::E_QKV>(t->XN1[l], C, P + lo.attn_w, C, M, 3 * C, C, epi_qkv(v.qkv, C, g->hs, g->nh, M * C))));
        MGPT_TRY(attn_forward_bf16(l, v));
        MGPT_TRY(branch_forward_bf16(SITE_ATTN_PROJ, l, all(), v.y, P + lo.proj_w, C, x, xm));
        return mlp_forward_bf16(l, all(), xm, x_out(l));
    }

    // backward: the MLP, then attention (model.py:50-71,102), c_attn and ln_1
    int layer_backward_f32(int l)
    {
        const LayerOff &lo = g->layers[l];
        const Tokens tk = all();
        MGPT_TRY(mlp_backward_f32(l, tk, true));                    // HT has held every later layer's gelu(a) since: recomputed
        MGPT_TRY(proj_backward_f32(l, tk, t->Y[l], t->DY));
        MGPT_TRY(attn_backward_f32(l, t->QKV[l], t->Y[l]));
        MGPT_TRY((tr_gemm<true, true, trk::OUT_STORE>(t->DQKV, 3 * C, P + lo.attn_w, C, t->DXN, C, M, C, 3 * C)));
        MGPT_TRY(weight_grad(t->DQKV, 3 * C, t->XN1[l], G + lo.attn_w, 3 * C, C, M));
        return ln_backward<true>(t->X[l], lo.ln1, tk);
    }

    int layer_backward_bf16(int l)
    {
        const LayerOff &lo = g->layers[l];
        const Tokens tk = all();
        const Bf16Layer v = bf16_layer(t, l, M, C);
        const Bf16Grads d = bf16_grads(t);
        MGPT_TRY(mlp_backward_bf16(l, tk));
        MGPT_TRY(proj_backward_bf16(l, tk, v.y, d.dy));
        MGPT_TRY(attn_backward_bf16(l, v, d.dy));
        MGPT_TRY((bf_gemm<float, true, float, false, tbk::E_F32>(t->DQKV, 3 * C, P + lo.attn_w, C, M, C, 3 * C, epi_f32(t->DXN, C))));
        MGPT_TRY(weight_grad_bf16(t->DQKV, 3 * C, t->XN1[l], G + lo.attn_w, 3 * C, C, M));
        return ln_backward<true>(t->X[l], lo.ln1, tk);
    }

    int layer_forward(int l) { return bf16 ? layer_forward_bf16(l) : layer_forward_f32(l); }
    int layer_backward(int l) { return bf16 ? layer_backward_bf16(l) : layer_backward_f32(l); }

    // ----- the last layer with its query, attention output, c_proj and MLP on the compact tokens (the rows call) -----
    // Of the last layer only ln_1 and the K | V projection run on all tokens.  Backward: the residual gradient is non-zero at token 255 only,
    // d K and d V are dense, so c_attn's K | V columns and ln_1 run over all tokens and everything else on the compact matrix.
    // Under dropout the compact tokens draw the general call's masks at token / query 255: site 1 through drop(SITE_ATTN, l) (the kernels
    // add query 255's offset), sites 2 and 3 through drop(site, l, k.tok).
    int gather_last(const float *src, float *dst, const Compact &k)
    {
        MGPT_LAUNCH(trk::gather_last_kernel, dim3(grid_1d((int64_t)k.mc * C)), dim3(256), 0, s, src, dst, k.n, k.mc, C);
        return MGPT_OK;
    }
    int scatter_last_add(const float *src, float *dst, const Compact &k)
    {
        MGPT_LAUNCH(trk::scatter_last_add_kernel, dim3(grid_1d((int64_t)k.n * C)), dim3(256), 0, s, src, dst, k.n, C);
        return MGPT_OK;
    }

    // fp32 forward: gemm_tr_kernel on the compact tokens
    int layer_forward_last_f32()
    {
        const int l = L - 1;
        const LayerOff &lo = g->layers[l];
        const Compact k = compact();
        const int64_t mc = k.mc;
        float *kp = t->QKV[l] + M * C, *vp = kp + M * C;
        MGPT_TRY(gpt_f32_layernorm(g, t->X[l], P + lo.ln1, t->XN1[l], M, s));
        MGPT_TRY(gpt_f32_linear(g, 2, t->XN1[l], P + lo.attn_w + (size_t)C * C, kp, M, 2 * C, C, s));           // k | v planes of every token
        MGPT_TRY(gather_last(t->XN1[l], k.xn1, k));
        MGPT_TRY(gather_last(t->X[l], k.x, k));
        MGPT_TRY((tr_gemm<true, false, trk::OUT_STORE>(k.xn1, C, P + lo.attn_w, C, k.q, C, mc, C, C)));
        MGPT_TRY(attn_last_forward<float>(k, k.q, kp, vp, k.y));
        MGPT_TRY(branch_forward_f32(SITE_ATTN_PROJ, l, k.tok, k.y, P + lo.proj_w, C, k.x, t->XM[l]));
        MGPT_TRY(gpt_f32_layernorm(g, t->XM[l], P + lo.ln2, t->XN2[l], mc, s));
        MGPT_TRY((tr_gemm<true, false, trk::OUT_STORE>(t->XN2[l], C, P + lo.fc_w, C, t->A[l], 4 * C, mc, 4 * C, C)));
        MGPT_TRY(gelu(l, k.tok));
        return branch_forward_f32(SITE_MLP_PROJ, l, k.tok, t->HT, P + lo.proj2_w, 4 * C, t->XM[l], t->XF);
    }

    int layer_forward_last_bf16()
    {
        const int l = L - 1;
        const LayerOff &lo = g->layers[l];
        const Compact k = compact();
        const Bf16Layer v = bf16_layer(t, l, k.mc, C);              // y, a, gelu(a) of the compact tokens; v.qkv: the compact q
        uint16_t *kp = v.qkv + M * C, *vp = kp + M * C;             // the general path's k and v planes
        MGPT_TRY(gpt_f32_layernorm(g, t->X[l], P + lo.ln1, t->XN1[l], M, s));
        MGPT_TRY((bf_gemm<float, true, float, true, tbk::E_QKV>(t->XN1[l], C, P + lo.attn_w + (size_t)C * C, C, M, 2 * C, C, epi_qkv(kp, C, g->hs, g->nh, M * C))));
        MGPT_TRY(gather_last(t->XN1[l], k.xn1, k));
        MGPT_TRY(gather_last(t->X[l], k.x, k));
        MGPT_TRY((bf_gemm<float, true, float, true, tbk::E_B16>(k.xn1, C, P + lo.attn_w, C, k.mc, C, C, epi_b16(v.qkv, C))));
        MGPT_TRY(attn_last_forward<uint16_t>(k, v.qkv, kp, vp, v.y));
        MGPT_TRY(branch_forward_bf16(SITE_ATTN_PROJ, l, k.tok, v.y, P + lo.proj_w, C, k.x, t->XM[l]));
        return mlp_forward_bf16(l, k.tok, t->XM[l], t->XF);
    }

    // the tail both precisions share: d ln_1(x) of token 255 joins DXN, ln_1 backward over all tokens, d x_mid of token 255 joins DX
    int layer_backward_last_tail(const Compact &k)
    {
        MGPT_TRY(scatter_last_add(k.dxn1, t->DXN, k));
        MGPT_TRY(ln_backward<false>(t->X[L - 1], g->layers[L - 1].ln1, all()));
        return scatter_last_add(k.tok.dx, t->DX, k);
    }

    // backward: the MLP and attention of query 255 -- d y, then d q (compact) and d k | d v (dense); c_attn: the K | V columns (from row kv
    // of its weight on) over all tokens, the Q rows from the compact tokens
    int layer_backward_last_f32()
    {
        const int l = L - 1;
        const LayerOff &lo = g->layers[l];
        const Compact k = compact();
        const int64_t mc = k.mc;
        const float *kp = t->QKV[l] + M * C, *vp = kp + M * C;
        const size_t kv = (size_t)C * C;
        MGPT_TRY(mlp_backward_f32(l, k.tok, false));                // HT still holds gelu(a) of the compact tokens: no layer ran after this one's forward
        MGPT_TRY(proj_backward_f32(l, k.tok, k.y, k.dy));
        MGPT_TRY(attn_last_backward<float>(k, k.q, kp, vp, k.y, k.dy));
        MGPT_TRY((tr_gemm<true, true, trk::OUT_STORE>(t->DQKV + C, 3 * C, P + lo.attn_w + kv, C, t->DXN, C, M, C, 2 * C)));
        MGPT_TRY((tr_gemm<true, true, trk::OUT_STORE>(k.dq, C, P + lo.attn_w, C, k.dxn1, C, mc, C, C)));
        MGPT_TRY(weight_grad(t->DQKV + C, 3 * C, t->XN1[l], G + lo.attn_w + kv, 2 * C, C, M));
        MGPT_TRY(weight_grad(k.dq, C, k.xn1, G + lo.attn_w, C, C, mc));
        return layer_backward_last_tail(k);
    }

    int layer_backward_last_bf16()
    {
        const int l = L - 1;
        const LayerOff &lo = g->layers[l];
        const Compact k = compact();
        const int64_t mc = k.mc;
        const Bf16Layer v = bf16_layer(t, l, mc, C);
        const Bf16Grads d = bf16_grads(t);                          // d.dy = k.dy's slot
        const uint16_t *kp = v.qkv + M * C, *vp = kp + M * C;
        const size_t kv = (size_t)C * C;
        MGPT_TRY(mlp_backward_bf16(l, k.tok));
        MGPT_TRY(proj_backward_bf16(l, k.tok, v.y, d.dy));
        MGPT_TRY(attn_last_backward<uint16_t>(k, v.qkv, kp, vp, v.y, d.dy));
        MGPT_TRY((bf_gemm<float, true, float, false, tbk::E_F32>(t->DQKV + C, 3 * C, P + lo.attn_w + kv, C, M, C, 2 * C, epi_f32(t->DXN, C))));
        MGPT_TRY((bf_gemm<float, true, float, false, tbk::E_F32>(k.dq, C, P + lo.attn_w, C, mc, C, C, epi_f32(k.dxn1, C))));
        MGPT_TRY(weight_grad_bf16(t->DQKV + C, 3 * C, t->XN1[l], G + lo.attn_w + kv, 2 * C, C, M));
        MGPT_TRY(weight_grad_bf16(k.dq, C, k.xn1, G + lo.attn_w, C, C, mc));
        return layer_backward_last_tail(k);
    }

    int layer_forward_last() { return bf16 ? layer_forward_last_bf16() : layer_forward_last_f32(); }
    int layer_backward_last() { return bf16 ? layer_backward_last_bf16() : layer_backward_last_f32(); }

    // ----- head (model.py:178-184), fp32 in both precisions: ln_f, logits = ln_f(x) @ wte^T, the caller's cross-entropy launch, the loss sum -----
    template <class CrossEntropy>
    int head_forward(const Tokens &tk, CrossEntropy cross_entropy)
    {
        MGPT_TRY(gpt_f32_layernorm(g, t->XF, P + g->off_lnf, t->XNF, tk.m, s));
        MGPT_TRY((tr_gemm<true, false, trk::OUT_STORE>(t->XNF, C, P + g->off_wte, C, t->LG, kV, tk.m, kV, C)));
        MGPT_TRY(cross_entropy());
        MGPT_LAUNCH(trk::sum_acc_kernel, dim3(1), dim3(256), 0, s, t->NLL, tk.m, t->loss_acc);
        return MGPT_OK;
    }
    // at every position against the call's target count (t->cnt), and of the compact tokens against call_rows, the row count of the WHOLE call
    int ce_targets()
    {
        MGPT_LAUNCH(trk::ce_kernel, dim3((unsigned)cdiv64(M, 256)), dim3(256), 0, s, t->LG, tg, M, t->cnt, loss_scale, t->DLG, t->NLL);
        return MGPT_OK;
    }
    int ce_rows(const Compact &k)
    {
        MGPT_LAUNCH(trk::ce_rows_kernel, dim3((unsigned)cdiv(k.mc, 256)), dim3(256), 0, s, (const float *)t->LG, tg, k.n, k.mc, loss_scale / (float)call_rows,
                    t->DLG, t->NLL);
        return MGPT_OK;
    }

    // d ln_f(x) = dlogits @ wte;  d wte += dlogits^T @ ln_f(x) (the tied lm_head);  ln_f backward starts the tokens' residual gradient dx
    int head_backward(const Tokens &tk)
    {
        MGPT_TRY((tr_gemm<true, true, trk::OUT_STORE>(t->DLG, kV, P + g->off_wte, C, tk.dxn, C, tk.m, C, kV)));
        MGPT_TRY(weight_grad(t->DLG, kV, t->XNF, G + g->off_wte, kV, C, tk.m));
        return ln_backward<false>(t->XF, g->off_lnf, tk);
    }

    // embedding (model.py:171-175), fp32 in both precisions: d wpe[t] += sum over rows, d wte[id] += sum over the tokens with that id
    // under dropout X[0] = m s (wte + wpe) (model.py:175) and the sums take m s DX (in DXN, free after the last LayerNorm backward)
    int embed()
    {
        MGPT_TRY(gpt_f32_embed(g, tok, t->X[0], M, s));
        return drops(SITE_EMBED) ? drop_scale(SITE_EMBED, 0, all(), t->X[0], t->X[0]) : MGPT_OK;
    }

    int embedding_backward()
    {
        const float *dx = t->DX;
        if (drops(SITE_EMBED)) {
            MGPT_TRY(drop_scale(SITE_EMBED, 0, all(), t->DX, t->DXN));
            dx = t->DXN;
        }
        MGPT_LAUNCH(trk::wpe_bwd_kernel, dim3((unsigned)cdiv64((int64_t)kT * C, 256)), dim3(256), 0, s, dx, rows, C, G + g->off_wpe);
        return slab_sum(G + g->off_wte, (int64_t)kV * C, 16, M, [&](int S, int kps) -> int {
            MGPT_LAUNCH(trk::wte_bwd_part_kernel, dim3(kV, (unsigned)S), dim3(256), 0, s, tok, dx, M, C, kps, t->part);
            return MGPT_OK;
        });
    }
};

// One chunk of rows: forward with saved activations, cross-entropy against the call's normaliser, backward into t->grads.  The rows call
// (c.call_rows > 0) runs the last layer and the head on the compact tokens; the layers below it are the general call's launches, masks
// included.  Slot lifetimes there: the dense fp32 forward's branch outputs pass through DY before the compact gradients live there, and
// branch_grad and embedding_backward fill DXN after layer_backward_last_tail has consumed it.
int chunk_fwd_bwd(Chunk &c)
{
    const bool last = c.call_rows > 0;
    const int dense = last ? c.L - 1 : c.L;
    const Compact k = c.compact();
    const Tokens head = last ? k.tok : c.all();
    MGPT_TRY(c.embed());
    for (int l = 0; l < dense; l++) MGPT_TRY(c.layer_forward(l));
    if (last) MGPT_TRY(c.layer_forward_last());
    MGPT_TRY(c.head_forward(head, [&]() -> int { return last ? c.ce_rows(k) : c.ce_targets(); }));
    MGPT_TRY(c.head_backward(head));
    if (last) MGPT_TRY(c.layer_backward_last());
    for (int l = dense - 1; l >= 0; l--) MGPT_TRY(c.layer_backward(l));
    return c.embedding_backward();
}

// the 16-bit threshold of sampling.py: dropout_threshold, and the kept elements' factor 1 / (1 - thr / 65536)
DropCfg drop_cfg(float p, uint64_t seed, uint64_t step, int sites)
{
    DropCfg dc;
    dc.thr = (uint32_t)std::min<long>(std::lround((double)p * 65536.0), 65535);
    dc.scale = 1.0f / (1.0f - (float)dc.thr / 65536.0f);
    dc.seed = seed; dc.step = step; dc.sites = sites;
    return dc;
}

int require_train(mgpt_gpt *g)
{
    MGPT_REQUIRE(g, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(g->train, MGPT_ERR_STATE, "no training workspace: mgpt_gpt_train_alloc first");
    return MGPT_OK;
}

// A micro-step call, general (call_rows = 0: d_aim the targets, 256 per row) or on rows (call_rows = rows: d_aim the labels, one per row).
// The checks both calls make, and the call's dropout; a call's own checks follow
int train_call_check(mgpt_gpt *g, const uint8_t *d_tokens, const int32_t *d_aim, int rows, int precision, float p, uint64_t seed, uint64_t step, int sites,
                     DropCfg *dc)
{
    MGPT_REQUIRE(p >= 0.f && p < 1.f, MGPT_ERR_ARG, "dropout p=%g: a probability in [0, 1)", (double)p);
    MGPT_REQUIRE(sites >= 0 && sites <= 15, MGPT_ERR_ARG, "dropout sites=%d: a mask of the four sites (15 = all, model.py's behaviour)", sites);
    MGPT_TRY(require_train(g));
    MGPT_REQUIRE(d_tokens && d_aim, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(rows > 0, MGPT_ERR_ARG, "rows=%d", rows);
    MGPT_REQUIRE(!g->has_bias, MGPT_ERR_UNSUPPORTED, "training supports bias = False checkpoints only (the released configs)");
    MGPT_REQUIRE(precision == MGPT_PREC_F32 || precision == MGPT_PREC_BF16, MGPT_ERR_UNSUPPORTED,
                 "training precision %d: MGPT_PREC_F32 (exact fp32) or MGPT_PREC_BF16 (bf16 mixed precision)", precision);
    MGPT_REQUIRE(ts(g)->max_rows > 0, MGPT_ERR_STATE, "the training workspace holds no activation memory (a re-size failed): mgpt_gpt_train_alloc again");
    *dc = drop_cfg(p, seed, step, sites);
    MGPT_REQUIRE(dc->thr == 0 || sites == 0 || g->C % 4 == 0, MGPT_ERR_UNSUPPORTED, "dropout masks come four elements to a hash: n_embd = %d is no multiple of 4", g->C);
    return MGPT_OK;
}

// ... and its chunks of at most max_rows rows into a zeroed loss sum: the masks are keyed by the row of the call, row0 + the chunk's first
int train_call_chunks(mgpt_gpt *g, const uint8_t *d_tokens, const int32_t *d_aim, int rows, int call_rows, float loss_scale, int precision, DropCfg dc,
                      uint64_t row0, hipStream_t s)
{
    TrainState *t = ts(g);
    MGPT_HIP(hipMemsetAsync(t->loss_acc, 0, sizeof(double), s));
    for (int r0 = 0; r0 < rows; r0 += t->max_rows) {
        dc.first_row = row0 + (uint64_t)r0;
        Chunk c = {g, t, d_tokens + (size_t)r0 * kT, d_aim + (size_t)r0 * (call_rows > 0 ? 1 : kT), std::min(t->max_rows, rows - r0), call_rows, loss_scale,
                   precision == MGPT_PREC_BF16, s, dc};
        MGPT_TRY(chunk_fwd_bwd(c));
    }
    return MGPT_OK;
}

}  // namespace

void gpt_train_destroy(mgpt_gpt *g)
{
    delete ts(g);                           // (its arenas free the workspace)
    g->train = nullptr;
}

extern "C" int mgpt_gpt_train_alloc(mgpt_gpt *g, int max_rows)
{
    MGPT_REQUIRE(g, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(max_rows > 0, MGPT_ERR_ARG, "max_rows=%d", max_rows);
    MGPT_REQUIRE(g->finalized, MGPT_ERR_STATE, "mgpt_gpt_finalize must precede mgpt_gpt_train_alloc");
    MGPT_REQUIRE(!g->has_bias, MGPT_ERR_UNSUPPORTED, "training supports bias = False checkpoints only (the released configs)");
    MGPT_REQUIRE(g->block == kT, MGPT_ERR_ARG, "training takes rows of T = 256 tokens; the model's block_size is %d", g->block);
    // the bf16 views of the workspace (bf16_layer): the statistics fit behind y, a and gelu(a) fit A[l]
    MGPT_REQUIRE(2 * g->nh <= g->C / 2, MGPT_ERR_UNSUPPORTED, "bf16 training keeps 2 n_head = %d statistics per token in the C / 2 = %d floats behind y",
                 2 * g->nh, g->C / 2);
    static_assert(2 * sizeof(uint16_t) <= sizeof(float), "bf16 a and gelu(a), 4 M C elements each, fit the 4 M C floats of A[l]");
    hipError_t e = hipSuccess;
    TrainState *t = ts(g);
    const bool fresh = t == nullptr;
    // an existing workspace keeps its gradients, AdamW moments and step counts: only the activation part is re-sized
    if (!fresh) {
        MGPT_HIP(hipDeviceSynchronize());              // (no queued call still uses the activations freed below)
        free_activations(t);
    } else {
        MGPT_TRY(g->hs == 32 ? raise_attn_lds<32>() : raise_attn_lds<64>());
        t = new TrainState();
    }
    auto alloc_in = [&](DeviceArena &owner, size_t bytes) -> void * {
        void *p = nullptr;
        if (e == hipSuccess) e = owner.alloc(&p, std::max<size_t>(bytes, 16));
        return p;
    };
    const int64_t M = (int64_t)max_rows * kT, C = g->C;
    const int L = g->L;
    const size_t nt = 3 + 6 * (size_t)L;
    if (fresh) {
        auto fp = [&](int64_t n) { return static_cast<float *>(alloc_in(t->mem, (size_t)n * sizeof(float))); };
        t->grads = fp(g->n_params); t->exp_avg = fp(g->n_params); t->exp_avg_sq = fp(g->n_params); t->steps = fp(nt);
        t->cnt = static_cast<int32_t *>(alloc_in(t->mem, 2 * sizeof(int32_t)));
        t->loss_acc = static_cast<double *>(alloc_in(t->mem, sizeof(double)));
        t->coef = fp(1);
        std::vector<trk::Blk> blk;
        const std::vector<TensorInfo> tt = tensor_table(g);
        for (size_t i = 0; i < tt.size(); i++)
            for (size_t b = 0; b < tt[i].count; b += trk::kChunk)
                blk.push_back({(int64_t)(tt[i].off + b), (int64_t)(tt[i].off + std::min(tt[i].count, b + trk::kChunk)), (int)i, tt[i].decay});
        t->n_blk = (int)blk.size();
        t->blk = static_cast<trk::Blk *>(alloc_in(t->mem, blk.size() * sizeof(trk::Blk)));
        t->norm_part = static_cast<double *>(alloc_in(t->mem, blk.size() * sizeof(double)));
        if (e == hipSuccess) e = t->mem.alloc_host(&t->h_cnt, 2 * sizeof(int32_t));
        if (e == hipSuccess) e = hipMemcpy(t->blk, blk.data(), blk.size() * sizeof(trk::Blk), hipMemcpyHostToDevice);
        for (float *p : {t->grads, t->exp_avg, t->exp_avg_sq})
            if (e == hipSuccess) e = hipMemset(p, 0, g->n_params * sizeof(float));
        if (e == hipSuccess) e = hipMemset(t->steps, 0, nt * sizeof(float));
        if (e != hipSuccess) {
            set_error("training workspace allocation failed: %s", hipGetErrorString(e));
            delete t;
            return MGPT_ERR_HIP;
        }
        g->train = t;
    }
    auto fa = [&](int64_t n) { return static_cast<float *>(alloc_in(t->act_mem, (size_t)n * sizeof(float))); };
    for (int l = 0; l < L; l++) {
        t->X.push_back(fa(M * C)); t->XN1.push_back(fa(M * C)); t->QKV.push_back(fa(3 * M * C)); t->Y.push_back(fa(M * C));
        t->XM.push_back(fa(M * C)); t->XN2.push_back(fa(M * C)); t->A.push_back(fa(4 * M * C));
    }
    t->XF = fa(M * C); t->XNF = fa(M * C); t->LG = fa(M * kV); t->DLG = fa(M * kV); t->NLL = fa(M);
    t->DX = fa(M * C); t->DXN = fa(M * C); t->DY = fa(M * C); t->DQKV = fa(3 * M * C); t->DH = fa(4 * M * C); t->HT = fa(4 * M * C);
    t->GP = fa(M * C); t->AST = fa(M * g->nh * 3);
    // weight-gradient, embedding and LayerNorm-gain partials (the bf16 path's: one row of C per 128 tokens)
    const size_t part_elems = std::max((size_t)slabs_of(M) * (size_t)std::max<int64_t>(4 * C * C, kV * C), (size_t)(cdiv64(M, tbk::kLnTok) * C));
    t->part = fa((int64_t)part_elems);
    if (e != hipSuccess) {             // the optimizer state survives; forward_backward refuses until a re-size succeeds
        set_error("training workspace allocation failed (%d rows): %s", max_rows, hipGetErrorString(e));
        free_activations(t);
        return MGPT_ERR_HIP;
    }
    t->part_elems = part_elems;
    t->max_rows = max_rows;
    t->M = M;
    return MGPT_OK;
}

extern "C" int mgpt_gpt_train_free(mgpt_gpt *g)
{
    MGPT_REQUIRE(g, MGPT_ERR_ARG, "NULL argument");
    gpt_train_destroy(g);
    return MGPT_OK;
}

extern "C" int mgpt_gpt_forward_backward(mgpt_gpt *g, const uint8_t *d_tokens, int rows, int T, const int32_t *d_targets, float loss_scale,
                                         float *d_loss, void *stream)
{
    return mgpt_gpt_forward_backward_prec(g, d_tokens, rows, T, d_targets, loss_scale, d_loss, MGPT_PREC_F32, stream);
}

extern "C" int mgpt_gpt_forward_backward_prec(mgpt_gpt *g, const uint8_t *d_tokens, int rows, int T, const int32_t *d_targets, float loss_scale,
                                              float *d_loss, int precision, void *stream)
{
    return mgpt_gpt_forward_backward_drop(g, d_tokens, rows, T, d_targets, loss_scale, d_loss, precision, 0.f, 0, 0, 0, 0, stream);
}

extern "C" int mgpt_gpt_forward_backward_drop(mgpt_gpt *g, const uint8_t *d_tokens, int rows, int T, const int32_t *d_targets, float loss_scale,
                                              float *d_loss, int precision, float p, uint64_t seed, uint64_t step, uint64_t row0, int sites,
                                              void *stream)
{
    DropCfg dc;
    MGPT_TRY(train_call_check(g, d_tokens, d_targets, rows, precision, p, seed, step, sites, &dc));
    MGPT_REQUIRE(T == kT, MGPT_ERR_ARG, "training takes rows of T = 256 tokens, got T = %d", T);
    TrainState *t = ts(g);
    hipStream_t s = (hipStream_t)stream;
    // the cross-entropy normaliser is the targeted-position count of the WHOLE call (F.cross_entropy's mean over the call's tokens)
    MGPT_LAUNCH(trk::count_targets_kernel, dim3(1), dim3(1024), 0, s, d_targets, (int64_t)rows * kT, t->cnt);
    MGPT_HIP(hipMemcpyAsync(t->h_cnt, t->cnt, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MGPT_HIP(hipStreamSynchronize(s));
    MGPT_REQUIRE(t->h_cnt[1] == 0, MGPT_ERR_ARG, "targets must lie in [-1, 67): -1 is ignored, 0 .. 66 are vocabulary ids");
    MGPT_REQUIRE(t->h_cnt[0] > 0, MGPT_ERR_ARG, "no targeted position in the call (every target is -1): the mean cross-entropy is undefined");
    MGPT_TRY(train_call_chunks(g, d_tokens, d_targets, rows, 0, loss_scale, precision, dc, row0, s));
    if (d_loss) MGPT_LAUNCH(trk::loss_final_kernel, dim3(1), dim3(64), 0, s, (const double *)t->loss_acc, t->cnt, d_loss);
    return MGPT_OK;
}

extern "C" int mgpt_gpt_forward_backward_rows(mgpt_gpt *g, const uint8_t *d_tokens, int rows, const int32_t *d_labels, float loss_scale,
                                              float *d_loss, int precision, void *stream)
{
    return mgpt_gpt_forward_backward_rows_drop(g, d_tokens, rows, d_labels, loss_scale, d_loss, precision, 0.f, 0, 0, 0, 0, stream);
}

extern "C" int mgpt_gpt_forward_backward_rows_drop(mgpt_gpt *g, const uint8_t *d_tokens, int rows, const int32_t *d_labels, float loss_scale,
                                                   float *d_loss, int precision, float p, uint64_t seed, uint64_t step, uint64_t row0, int sites,
                                                   void *stream)
{
    DropCfg dc;
    MGPT_TRY(train_call_check(g, d_tokens, d_labels, rows, precision, p, seed, step, sites, &dc));
    MGPT_REQUIRE(std::isfinite(loss_scale), MGPT_ERR_ARG, "loss_scale=%g: a finite factor", (double)loss_scale);
    hipStream_t s = (hipStream_t)stream;
    // every launch is stream-ordered and the normaliser is `rows`: the host waits for nothing
    MGPT_TRY(train_call_chunks(g, d_tokens, d_labels, rows, rows, loss_scale, precision, dc, row0, s));
    if (d_loss) MGPT_LAUNCH(trk::loss_final_rows_kernel, dim3(1), dim3(64), 0, s, (const double *)ts(g)->loss_acc, (double)rows, d_loss);
    return MGPT_OK;
}

extern "C" int mgpt_gpt_zero_grad(mgpt_gpt *g, void *stream)
{
    MGPT_TRY(require_train(g));
    MGPT_HIP(hipMemsetAsync(ts(g)->grads, 0, g->n_params * sizeof(float), (hipStream_t)stream));
    return MGPT_OK;
}

// ----- data-parallel gradient synchronisation (train.py:237-239, 314-322): the whole buffer out, the ranks' buffers summed in rank order -----
extern "C" int mgpt_gpt_grads_size(mgpt_gpt *g, int64_t *n_elem)
{
    MGPT_REQUIRE(g && n_elem, MGPT_ERR_ARG, "NULL argument");
    MGPT_TRY(require_train(g));
    *n_elem = (int64_t)g->n_params;
    return MGPT_OK;
}

extern "C" int mgpt_gpt_grads_export(mgpt_gpt *g, float *d_out, int64_t n_elem, void *stream)
{
    MGPT_REQUIRE(g && d_out, MGPT_ERR_ARG, "NULL argument");
    MGPT_TRY(require_train(g));
    MGPT_REQUIRE(n_elem == (int64_t)g->n_params, MGPT_ERR_ARG, "the gradient buffer has %zu elements, got %lld", g->n_params, (long long)n_elem);
    MGPT_HIP(hipMemcpyAsync(d_out, ts(g)->grads, g->n_params * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGPT_OK;
}

extern "C" int mgpt_gpt_grads_reduce(mgpt_gpt *g, const float *d_gathered, int world, float scale, void *stream)
{
    MGPT_REQUIRE(g && d_gathered, MGPT_ERR_ARG, "NULL argument");
    MGPT_TRY(require_train(g));
    MGPT_REQUIRE(world >= 1, MGPT_ERR_ARG, "world=%d", world);
    MGPT_REQUIRE(std::isfinite(scale) && scale > 0.f, MGPT_ERR_ARG, "scale=%g: a finite positive factor (1 / world for the ranks' mean)", scale);
    TrainState *t = ts(g);
    const int64_t n = (int64_t)g->n_params;
    // 16-byte accesses need every row of d_gathered and the gradient buffer on a 16-byte boundary; otherwise the scalar loop takes it all
    const bool wide = n % 4 == 0 && reinterpret_cast<uintptr_t>(d_gathered) % 16 == 0 && reinterpret_cast<uintptr_t>(t->grads) % 16 == 0;
    const int64_t nv = wide ? n / 4 : 0;
    MGPT_LAUNCH(trk::rank_reduce_kernel, dim3(grid_1d(wide ? nv : n)), dim3(256), 0, (hipStream_t)stream, d_gathered, world, n, nv, scale, t->grads);
    return MGPT_OK;
}

extern "C" int mgpt_gpt_clip_grad_norm(mgpt_gpt *g, float max_norm, float *d_total_norm, void *stream)
{
    MGPT_TRY(require_train(g));
    TrainState *t = ts(g);
    hipStream_t s = (hipStream_t)stream;
    MGPT_LAUNCH(trk::sumsq_part_kernel, dim3((unsigned)t->n_blk), dim3(256), 0, s, t->grads, (const trk::Blk *)t->blk, t->norm_part);
    MGPT_LAUNCH(trk::clip_coef_kernel, dim3(1), dim3(64), 0, s, (const double *)t->norm_part, (const trk::Blk *)t->blk, t->n_blk, max_norm > 0.f ? max_norm : 1.f,
                d_total_norm, t->coef);
    if (max_norm > 0.f) MGPT_LAUNCH(trk::scale_kernel, dim3(grid_1d((int64_t)g->n_params)), dim3(256), 0, s, t->grads, (int64_t)g->n_params, t->coef);
    return MGPT_OK;
}

extern "C" int mgpt_gpt_adamw_step(mgpt_gpt *g, float lr, float beta1, float beta2, float eps, float weight_decay, void *stream)
{
    MGPT_TRY(require_train(g));
    MGPT_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && lr >= 0.f, MGPT_ERR_ARG,
                 "AdamW hyper-parameters out of range (lr %g, betas %g %g, eps %g)", lr, beta1, beta2, eps);
    TrainState *t = ts(g);
    hipStream_t s = (hipStream_t)stream;
    const int nt = 3 + 6 * g->L;
    MGPT_LAUNCH(trk::step_inc_kernel, dim3((unsigned)cdiv(nt, 256)), dim3(256), 0, s, t->steps, nt);
    MGPT_LAUNCH(trk::adamw_kernel, dim3((unsigned)t->n_blk), dim3(256), 0, s, g->params, t->grads, t->exp_avg, t->exp_avg_sq, (const trk::Blk *)t->blk, t->steps, lr,
                beta1, beta2, eps, weight_decay);
    gpt_params_changed(g);
    return MGPT_OK;
}

// which: MGPT_TRAIN_PARAM, _GRAD, _EXP_AVG, _EXP_AVG_SQ (the tensor's elements), _STEP (one float)
static int train_locate(mgpt_gpt *g, const char *name, int which, float **ptr, size_t *count)
{
    size_t idx, off, cnt;
    MGPT_REQUIRE(name && gpt_locate_param(g, name, &idx, &off, &cnt), MGPT_ERR_ARG, "unknown parameter '%s'", name ? name : "(null)");
    if (which == MGPT_TRAIN_PARAM) { *ptr = g->params + off; *count = cnt; return MGPT_OK; }     // (no workspace needed)
    TrainState *t = ts(g);
    MGPT_REQUIRE(t, MGPT_ERR_STATE, "no training workspace: mgpt_gpt_train_alloc first");
    switch (which) {
        case MGPT_TRAIN_GRAD: *ptr = t->grads + off; *count = cnt; return MGPT_OK;
        case MGPT_TRAIN_EXP_AVG: *ptr = t->exp_avg + off; *count = cnt; return MGPT_OK;
        case MGPT_TRAIN_EXP_AVG_SQ: *ptr = t->exp_avg_sq + off; *count = cnt; return MGPT_OK;
        case MGPT_TRAIN_STEP: *ptr = t->steps + idx; *count = 1; return MGPT_OK;
        default: break;
    }
    set_error("which=%d", which);
    return MGPT_ERR_ARG;
}

extern "C" int mgpt_gpt_train_get(mgpt_gpt *g, const char *name, int which, float *d_out, int64_t n_elem, void *stream)
{
    MGPT_REQUIRE(g && d_out, MGPT_ERR_ARG, "NULL argument");
    float *src = nullptr;
    size_t count = 0;
    MGPT_TRY(train_locate(g, name, which, &src, &count));
    MGPT_REQUIRE((size_t)n_elem == count, MGPT_ERR_ARG, "'%s' (which %d): got %lld elements, expected %zu", name, which, (long long)n_elem, count);
    MGPT_HIP(hipMemcpyAsync(d_out, src, count * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGPT_OK;
}

extern "C" int mgpt_gpt_train_set(mgpt_gpt *g, const char *name, int which, const float *data, int64_t n_elem, int is_device)
{
    MGPT_REQUIRE(g && data, MGPT_ERR_ARG, "NULL argument");
    float *dst = nullptr;
    size_t count = 0;
    MGPT_TRY(train_locate(g, name, which, &dst, &count));
    MGPT_REQUIRE((size_t)n_elem == count, MGPT_ERR_ARG, "'%s' (which %d): got %lld elements, expected %zu", name, which, (long long)n_elem, count);
    MGPT_HIP(hipDeviceSynchronize());                  // (stream-ordered work on the tensor finishes first: this call is synchronous)
    MGPT_HIP(hipMemcpy(dst, data, count * sizeof(float), is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    if (which == MGPT_TRAIN_PARAM) gpt_params_changed(g);
    return MGPT_OK;
}
