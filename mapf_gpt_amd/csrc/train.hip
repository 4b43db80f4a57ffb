// train.hip -- training on the device (replaces train.py:324-331 with model.py:180-184 and :202-226): exact-fp32 or bf16 mixed-precision
// forward with saved activations, backward into one fp32 gradient buffer in the layout of mgpt_gpt::params, torch's clip_grad_norm_ and AdamW.
#include <string>
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
    float *DX = nullptr, *DXN = nullptr, *DY = nullptr, *DQKV = nullptr, *DH = nullptr, *HT = nullptr, *GP = nullptr, *AST = nullptr;
    float *part = nullptr;                  // weight-gradient / gain / embedding slabs
    size_t part_elems = 0;
    int32_t *cnt = nullptr;                 // [0] targeted positions of the call, [1] invalid-target flag
    int32_t *h_cnt = nullptr;               // pinned host copy
    double *loss_acc = nullptr;
    float *coef = nullptr;
    trk::Blk *blk = nullptr;
    int n_blk = 0;
    double *norm_part = nullptr;
    std::vector<void *> allocs;             // gradients, AdamW state and bookkeeping: live as long as the workspace
    std::vector<void *> act_allocs;         // activations and backward scratch of max_rows rows: re-sized by mgpt_gpt_train_alloc
};

TrainState *ts(mgpt_gpt *g) { return static_cast<TrainState *>(g->train); }

void free_activations(TrainState *t)
{
    for (void *p : t->act_allocs) (void)hipFree(p);
    t->act_allocs.clear();
    t->X.clear(); t->XN1.clear(); t->QKV.clear(); t->Y.clear(); t->XM.clear(); t->XN2.clear(); t->A.clear();
    t->max_rows = 0;
    t->M = 0;
    t->part_elems = 0;
}

void free_state(TrainState *t)
{
    free_activations(t);
    for (void *p : t->allocs) (void)hipFree(p);
    if (t->h_cnt) (void)hipHostFree(t->h_cnt);
    delete t;
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

int slabs_of(int64_t M) { return (int)std::min<int64_t>(kMaxSlabs, std::max<int64_t>(1, cdiv64(M, kSlabTokens))); }
int slab_tokens(int64_t M) { const int S = slabs_of(M); return (int)((cdiv64(M, S) + 15) / 16 * 16); }

unsigned grid_1d(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n, 256), 8192)); }

// ----- backward pieces -----
// out[M][N] (op)= A'(M x K) @ B'(K x N) over all K
template <bool A_KC, bool B_NC, int OUT>
int tr_gemm(const float *A, int64_t lda, const float *B, int64_t ldb, float *out, int64_t ldc, int64_t M, int N, int K, hipStream_t s,
            const float *aux = nullptr)
{
    const dim3 grid((unsigned)cdiv(N, 64), (unsigned)cdiv64(M, 64), 1);
    hipLaunchKernelGGL((trk::gemm_tr_kernel<A_KC, B_NC, OUT>), grid, dim3(256), 0, s, A, lda, B, ldb, out, ldc, (int)M, N, K, K, aux);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// dW[Nout][Kin] += dY^T @ X over Mtok tokens: dY [Mtok][Nout], X [Mtok][Kin]; slabs of tokens, summed in order
int weight_grad(TrainState *t, const float *dY, const float *X, float *dW, int Nout, int Kin, int64_t Mtok, hipStream_t s)
{
    const int S = slabs_of(Mtok), kps = slab_tokens(Mtok);
    MGPT_REQUIRE((size_t)S * Nout * Kin <= t->part_elems, MGPT_ERR_ARG, "weight-gradient slabs exceed the workspace");
    const dim3 grid((unsigned)cdiv(Kin, 64), (unsigned)cdiv(Nout, 64), (unsigned)S);
    hipLaunchKernelGGL((trk::gemm_tr_kernel<false, true, trk::OUT_PART>), grid, dim3(256), 0, s, dY, (int64_t)Nout, X, (int64_t)Kin, t->part,
                       (int64_t)Kin, Nout, Kin, (int)Mtok, kps, (const float *)nullptr);
    MGPT_LAUNCH_CHECK();
    const int64_t n = (int64_t)Nout * Kin;
    hipLaunchKernelGGL(trk::slab_reduce_kernel, dim3(grid_1d(n)), dim3(256), 0, s, t->part, S, n, dW);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// LayerNorm backward: dres (+)= d x, gain gradient += sum_m dxn * xhat
template <bool ADD>
int ln_backward(TrainState *t, const float *x, const float *w, const float *dxn, float *dres, float *gw, int64_t Mtok, int C, hipStream_t s)
{
    hipLaunchKernelGGL((trk::ln_bwd_kernel<ADD>), dim3((unsigned)cdiv64(Mtok, 4)), dim3(256), 0, s, x, w, dxn, dres, t->GP, Mtok, C);
    MGPT_LAUNCH_CHECK();
    const int S = slabs_of(Mtok), kps = slab_tokens(Mtok);
    hipLaunchKernelGGL(trk::colsum_part_kernel, dim3((unsigned)cdiv(C, 256), (unsigned)S), dim3(256), 0, s, t->GP, Mtok, C, kps, t->part);
    MGPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(trk::slab_reduce_kernel, dim3(grid_1d(C)), dim3(256), 0, s, t->part, S, (int64_t)C, gw);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

template <int HS>
int attn_backward(mgpt_gpt *g, TrainState *t, const float *qkv, int64_t plane, const float *Y, int rows, float scale, hipStream_t s)
{
    const size_t lds_q = (size_t)2 * kT * HS * sizeof(float), lds_kv = lds_q + (size_t)3 * kT * sizeof(float);
    MGPT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&trk::attn_bwd_q_kernel<HS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_q));
    MGPT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&trk::attn_bwd_kv_kernel<HS, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_kv));
    MGPT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&trk::attn_bwd_kv_kernel<HS, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_kv));
    const dim3 grid((unsigned)(rows * g->nh));
    hipLaunchKernelGGL(trk::attn_bwd_q_kernel<HS>, grid, dim3(256), lds_q, s, qkv, plane, Y, (const float *)t->DY, t->DQKV, t->AST, g->nh, scale);
    MGPT_LAUNCH_CHECK();
    hipLaunchKernelGGL((trk::attn_bwd_kv_kernel<HS, 0>), grid, dim3(256), lds_kv, s, qkv, plane, (const float *)t->DY, t->DQKV, (const float *)t->AST, g->nh, scale);
    MGPT_LAUNCH_CHECK();
    hipLaunchKernelGGL((trk::attn_bwd_kv_kernel<HS, 1>), grid, dim3(256), lds_kv, s, qkv, plane, (const float *)t->DY, t->DQKV, (const float *)t->AST, g->nh, scale);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// one chunk of rows: forward with saved activations, cross-entropy against the call's target count, backward into t->grads
int chunk_fwd_bwd(mgpt_gpt *g, TrainState *t, const uint8_t *tok, int rows, const int32_t *tg, float loss_scale, hipStream_t s)
{
    const int C = g->C, L = g->L;
    const int64_t M = (int64_t)rows * kT;
    const float *P = g->params;
    float *G = t->grads;
    int rc;
    if ((rc = gpt_f32_embed(g, tok, t->X[0], M, s)) != MGPT_OK) return rc;
    const float scale = 1.0f / sqrtf((float)g->hs);
    for (int l = 0; l < L; l++) {
        const LayerOff &lo = g->layers[l];
        float *x = t->X[l], *xm = t->XM[l], *xo = (l + 1 < L) ? t->X[l + 1] : t->XF;
        if ((rc = gpt_f32_layernorm(g, x, P + lo.ln1, t->XN1[l], M, s)) != MGPT_OK) return rc;
        if ((rc = gpt_f32_linear(g, 2, t->XN1[l], P + lo.attn_w, t->QKV[l], M, 3 * C, C, s)) != MGPT_OK) return rc;
        if ((rc = gpt_f32_attention(g, t->QKV[l], t->Y[l], rows, s)) != MGPT_OK) return rc;
        MGPT_HIP(hipMemcpyAsync(xm, x, (size_t)M * C * sizeof(float), hipMemcpyDeviceToDevice, s));
        if ((rc = gpt_f32_linear(g, 1, t->Y[l], P + lo.proj_w, xm, M, C, C, s)) != MGPT_OK) return rc;
        if ((rc = gpt_f32_layernorm(g, xm, P + lo.ln2, t->XN2[l], M, s)) != MGPT_OK) return rc;
        if ((rc = gpt_f32_linear(g, 0, t->XN2[l], P + lo.fc_w, t->A[l], M, 4 * C, C, s)) != MGPT_OK) return rc;
        hipLaunchKernelGGL(trk::gelu_kernel, dim3(grid_1d(4 * M * C)), dim3(256), 0, s, (const float *)t->A[l], t->HT, 4 * M * C);
        MGPT_LAUNCH_CHECK();
        MGPT_HIP(hipMemcpyAsync(xo, xm, (size_t)M * C * sizeof(float), hipMemcpyDeviceToDevice, s));
        if ((rc = gpt_f32_linear(g, 1, t->HT, P + lo.proj2_w, xo, M, C, 4 * C, s)) != MGPT_OK) return rc;
    }
    // head (model.py:178-184): ln_f, logits = ln_f(x) @ wte^T at every position, cross-entropy
    if ((rc = gpt_f32_layernorm(g, t->XF, P + g->off_lnf, t->XNF, M, s)) != MGPT_OK) return rc;
    if ((rc = tr_gemm<true, false, trk::OUT_STORE>(t->XNF, C, P + g->off_wte, C, t->LG, kV, M, kV, C, s)) != MGPT_OK) return rc;
    hipLaunchKernelGGL(trk::ce_kernel, dim3((unsigned)cdiv64(M, 256)), dim3(256), 0, s, (const float *)t->LG, tg, M, (const int32_t *)t->cnt,
                       loss_scale, t->DLG, t->NLL);
    MGPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(trk::sum_acc_kernel, dim3(1), dim3(256), 0, s, (const float *)t->NLL, M, t->loss_acc);
    MGPT_LAUNCH_CHECK();
    // d ln_f(x) = dlogits @ wte;  d wte += dlogits^T @ ln_f(x) (the tied lm_head);  ln_f backward starts the residual gradient
    if ((rc = tr_gemm<true, true, trk::OUT_STORE>(t->DLG, kV, P + g->off_wte, C, t->DXN, C, M, C, kV, s)) != MGPT_OK) return rc;
    if ((rc = weight_grad(t, t->DLG, t->XNF, G + g->off_wte, kV, C, M, s)) != MGPT_OK) return rc;
    if ((rc = ln_backward<false>(t, t->XF, P + g->off_lnf, t->DXN, t->DX, G + g->off_lnf, M, C, s)) != MGPT_OK) return rc;
    for (int l = L - 1; l >= 0; l--) {
        const LayerOff &lo = g->layers[l];
        // MLP (model.py:85-87,103): DX = d x_out
        if ((rc = tr_gemm<true, true, trk::OUT_GELU_BWD>(t->DX, C, P + lo.proj2_w, 4 * C, t->DH, 4 * C, M, 4 * C, C, s, t->A[l])) != MGPT_OK) return rc;
        hipLaunchKernelGGL(trk::gelu_kernel, dim3(grid_1d(4 * M * C)), dim3(256), 0, s, (const float *)t->A[l], t->HT, 4 * M * C);
        MGPT_LAUNCH_CHECK();
        if ((rc = weight_grad(t, t->DX, t->HT, G + lo.proj2_w, C, 4 * C, M, s)) != MGPT_OK) return rc;
        if ((rc = tr_gemm<true, true, trk::OUT_STORE>(t->DH, 4 * C, P + lo.fc_w, C, t->DXN, C, M, C, 4 * C, s)) != MGPT_OK) return rc;
        if ((rc = weight_grad(t, t->DH, t->XN2[l], G + lo.fc_w, 4 * C, C, M, s)) != MGPT_OK) return rc;
        if ((rc = ln_backward<true>(t, t->XM[l], P + lo.ln2, t->DXN, t->DX, G + lo.ln2, M, C, s)) != MGPT_OK) return rc;
        // attention (model.py:50-71,102): DX = d x_mid
        if ((rc = tr_gemm<true, true, trk::OUT_STORE>(t->DX, C, P + lo.proj_w, C, t->DY, C, M, C, C, s)) != MGPT_OK) return rc;
        if ((rc = weight_grad(t, t->DX, t->Y[l], G + lo.proj_w, C, C, M, s)) != MGPT_OK) return rc;
        rc = g->hs == 32 ? attn_backward<32>(g, t, t->QKV[l], M * C, t->Y[l], rows, scale, s)
                         : attn_backward<64>(g, t, t->QKV[l], M * C, t->Y[l], rows, scale, s);
        if (rc != MGPT_OK) return rc;
        if ((rc = tr_gemm<true, true, trk::OUT_STORE>(t->DQKV, 3 * C, P + lo.attn_w, C, t->DXN, C, M, C, 3 * C, s)) != MGPT_OK) return rc;
        if ((rc = weight_grad(t, t->DQKV, t->XN1[l], G + lo.attn_w, 3 * C, C, M, s)) != MGPT_OK) return rc;
        if ((rc = ln_backward<true>(t, t->X[l], P + lo.ln1, t->DXN, t->DX, G + lo.ln1, M, C, s)) != MGPT_OK) return rc;
    }
    // embedding (model.py:171-175): d wpe[t] += sum over rows, d wte[id] += sum over the tokens with that id
    hipLaunchKernelGGL(trk::wpe_bwd_kernel, dim3((unsigned)cdiv64((int64_t)kT * C, 256)), dim3(256), 0, s, (const float *)t->DX, rows, C, G + g->off_wpe);
    MGPT_LAUNCH_CHECK();
    {
        const int S = slabs_of(M), kps = slab_tokens(M);
        hipLaunchKernelGGL(trk::wte_bwd_part_kernel, dim3(kV, (unsigned)S), dim3(256), 0, s, tok, (const float *)t->DX, M, C, kps, t->part);
        MGPT_LAUNCH_CHECK();
        hipLaunchKernelGGL(trk::slab_reduce_kernel, dim3(grid_1d((int64_t)kV * C)), dim3(256), 0, s, t->part, S, (int64_t)kV * C, G + g->off_wte);
        MGPT_LAUNCH_CHECK();
    }
    return MGPT_OK;
}

// ----- bf16 mixed precision (MGPT_PREC_BF16): the matrix products of the five linears on bf16 MFMAs (gpt_kernels_train_bf16.h) -----
int gemm_bf16_check(int64_t M, int N, int K, int kps)
{
    MGPT_REQUIRE(M % 16 == 0 && N % 16 == 0 && K % 32 == 0 && kps % 32 == 0 && M <= INT32_MAX, MGPT_ERR_UNSUPPORTED,
                 "bf16 gemm shape M=%lld N=%d K=%d (slab %d)", (long long)M, N, K, kps);
    return MGPT_OK;
}

template <typename TA, bool A_KC, typename TB, bool B_KC, int EPI>
int bf_gemm(const TA *A, int64_t lda, const TB *B, int64_t ldb, int64_t M, int N, int K, const tbk::Epi &ep, hipStream_t s, int slabs = 1,
            int kps = 0)
{
    if (slabs == 1) kps = K;
    const int rc = gemm_bf16_check(M, N, K, kps);
    if (rc != MGPT_OK) return rc;
    const dim3 grid((unsigned)cdiv(N, tbk::BN), (unsigned)cdiv64(M, tbk::BM), (unsigned)slabs);
    hipLaunchKernelGGL((tbk::gemm_bf16_kernel<TA, A_KC, TB, B_KC, EPI>), grid, dim3(256), 0, s, A, lda, B, ldb, (int)M, N, K, kps, ep);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// dW[Nout][Kin] += dY^T @ X over Mtok tokens on bf16 MFMAs: fp32 partials per token slab (the slabs of weight_grad, 32-token aligned), summed in order
template <typename TY, typename TX>
int weight_grad_bf16(TrainState *t, const TY *dY, const TX *X, float *dW, int Nout, int Kin, int64_t Mtok, hipStream_t s)
{
    const int S = slabs_of(Mtok), kps = (int)((cdiv64(Mtok, S) + 31) / 32 * 32);
    MGPT_REQUIRE((size_t)S * Nout * Kin <= t->part_elems, MGPT_ERR_ARG, "weight-gradient slabs exceed the workspace");
    tbk::Epi ep;
    ep.f32 = t->part;
    ep.ldc = Kin;
    int rc = bf_gemm<TY, false, TX, false, tbk::E_PART>(dY, Nout, X, Kin, Nout, Kin, (int)Mtok, ep, s, S, kps);
    if (rc != MGPT_OK) return rc;
    const int64_t n = (int64_t)Nout * Kin;
    hipLaunchKernelGGL(trk::slab_reduce_kernel, dim3(grid_1d(n)), dim3(256), 0, s, (const float *)t->part, S, n, dW);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// LayerNorm backward with the gain's column sums fused: one partial per 128 tokens, summed in order
template <bool ADD>
int ln_backward_bf16(TrainState *t, const float *x, const float *w, const float *dxn, float *dres, float *gw, int64_t Mtok, int C, hipStream_t s)
{
    const int64_t P = cdiv64(Mtok, tbk::kLnTok);
    MGPT_REQUIRE(C <= 64 * tbk::kLnMaxJ && (size_t)(P * C) <= t->part_elems, MGPT_ERR_UNSUPPORTED, "LayerNorm backward: C=%d, %lld tokens", C,
                 (long long)Mtok);
    hipLaunchKernelGGL((tbk::ln_bwd_gain_kernel<ADD>), dim3((unsigned)P), dim3(256), 0, s, x, w, dxn, dres, t->part, Mtok, C);
    MGPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tbk::colsum_reduce_kernel, dim3((unsigned)cdiv(C, 64)), dim3(1024), 0, s, (const float *)t->part, (int)P, C, gw);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// attention on bf16 MFMAs: forward (y bf16, statistics fp32) and backward (dq | dk | dv fp32 into t->DQKV)
template <int HS>
int attn_bf16(const uint16_t *qkv, int64_t plane, uint16_t *y, float *stats, int rows, int n_head, float scale, hipStream_t s)
{
    const size_t lds = tbk::attn_fwd_lds<HS>();
    MGPT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&tbk::attn_fwd_bf16_kernel<HS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(tbk::attn_fwd_bf16_kernel<HS>, dim3((unsigned)(rows * n_head)), dim3(256), lds, s, qkv, plane, y, stats, n_head, scale);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

template <int HS>
int attn_bwd_bf16(TrainState *t, const uint16_t *qkv, int64_t plane, const uint16_t *y, const uint16_t *dy, const float *stats, int rows,
                  int n_head, float scale, hipStream_t s)
{
    const size_t lds = tbk::attn_bwd_lds<HS>();
    MGPT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&tbk::attn_bwd_bf16_kernel<HS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(tbk::attn_bwd_bf16_kernel<HS>, dim3((unsigned)(rows * n_head)), dim3(512), lds, s, qkv, plane, y, dy, stats, t->DQKV,
                       n_head, scale);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// one chunk of rows in train.py's autocast regime.  Rounded to bf16 (as autocast holds them): the operands of the five linears -- the head's
// excepted, which stays fp32 --, q, k, v, attention's output and its gradient, P and dS, the linears' outputs and GELU's, the gradients of the
// MLP hidden tensors.  fp32: the embedding sum, the residual stream and its gradient, LayerNorm, softmax statistics, cross-entropy and every
// accumulator.  The workspace is the fp32 path's: QKV[l] holds the bf16 q | k | v planes, Y[l] bf16 y and then the softmax statistics, A[l]
// bf16(a) | bf16(gelu(a)), DY the bf16 gradient of y, DH the bf16 gradient of a.
int chunk_fwd_bwd_bf16(mgpt_gpt *g, TrainState *t, const uint8_t *tok, int rows, const int32_t *tg, float loss_scale, hipStream_t s)
{
    const int C = g->C, L = g->L;
    const int64_t M = (int64_t)rows * kT;
    const float *P = g->params;
    float *G = t->grads;
    int rc;
    tbk::Epi ep;
    if ((rc = gpt_f32_embed(g, tok, t->X[0], M, s)) != MGPT_OK) return rc;
    const float scale = 1.0f / sqrtf((float)g->hs);
    for (int l = 0; l < L; l++) {
        const LayerOff &lo = g->layers[l];
        float *x = t->X[l], *xm = t->XM[l], *xo = (l + 1 < L) ? t->X[l + 1] : t->XF;
        uint16_t *a16 = reinterpret_cast<uint16_t *>(t->A[l]), *h16 = a16 + 4 * M * C;
        uint16_t *qkv16 = reinterpret_cast<uint16_t *>(t->QKV[l]), *y16 = reinterpret_cast<uint16_t *>(t->Y[l]);
        float *ast = reinterpret_cast<float *>(y16 + M * C);          // 2 n_head floats per token <= the C / 2 floats left in Y[l]
        if ((rc = gpt_f32_layernorm(g, x, P + lo.ln1, t->XN1[l], M, s)) != MGPT_OK) return rc;
        ep = tbk::Epi();
        ep.b16 = qkv16; ep.C = C; ep.hs = g->hs; ep.n_head = g->nh; ep.plane = M * C;
        if ((rc = bf_gemm<float, true, float, true, tbk::E_QKV>(t->XN1[l], C, P + lo.attn_w, C, M, 3 * C, C, ep, s)) != MGPT_OK) return rc;
        rc = g->hs == 32 ? attn_bf16<32>(qkv16, M * C, y16, ast, rows, g->nh, scale, s)
                         : attn_bf16<64>(qkv16, M * C, y16, ast, rows, g->nh, scale, s);
        if (rc != MGPT_OK) return rc;
        ep = tbk::Epi();
        ep.f32 = xm; ep.res = x; ep.ldc = C;
        if ((rc = bf_gemm<uint16_t, true, float, true, tbk::E_RESID>(y16, C, P + lo.proj_w, C, M, C, C, ep, s)) != MGPT_OK) return rc;
        if ((rc = gpt_f32_layernorm(g, xm, P + lo.ln2, t->XN2[l], M, s)) != MGPT_OK) return rc;
        ep = tbk::Epi();
        ep.b16 = a16; ep.b16b = h16; ep.ldc = 4 * C;
        if ((rc = bf_gemm<float, true, float, true, tbk::E_FC>(t->XN2[l], C, P + lo.fc_w, C, M, 4 * C, C, ep, s)) != MGPT_OK) return rc;
        ep = tbk::Epi();
        ep.f32 = xo; ep.res = xm; ep.ldc = C;
        if ((rc = bf_gemm<uint16_t, true, float, true, tbk::E_RESID>(h16, 4 * C, P + lo.proj2_w, 4 * C, M, C, 4 * C, ep, s)) != MGPT_OK) return rc;
    }
    // head: the fp32 path's (ln_f, the tied head in fp32, cross-entropy), with this path's LayerNorm backward
    if ((rc = gpt_f32_layernorm(g, t->XF, P + g->off_lnf, t->XNF, M, s)) != MGPT_OK) return rc;
    if ((rc = tr_gemm<true, false, trk::OUT_STORE>(t->XNF, C, P + g->off_wte, C, t->LG, kV, M, kV, C, s)) != MGPT_OK) return rc;
    hipLaunchKernelGGL(trk::ce_kernel, dim3((unsigned)cdiv64(M, 256)), dim3(256), 0, s, (const float *)t->LG, tg, M, (const int32_t *)t->cnt,
                       loss_scale, t->DLG, t->NLL);
    MGPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(trk::sum_acc_kernel, dim3(1), dim3(256), 0, s, (const float *)t->NLL, M, t->loss_acc);
    MGPT_LAUNCH_CHECK();
    if ((rc = tr_gemm<true, true, trk::OUT_STORE>(t->DLG, kV, P + g->off_wte, C, t->DXN, C, M, C, kV, s)) != MGPT_OK) return rc;
    if ((rc = weight_grad(t, t->DLG, t->XNF, G + g->off_wte, kV, C, M, s)) != MGPT_OK) return rc;
    if ((rc = ln_backward_bf16<false>(t, t->XF, P + g->off_lnf, t->DXN, t->DX, G + g->off_lnf, M, C, s)) != MGPT_OK) return rc;
    for (int l = L - 1; l >= 0; l--) {
        const LayerOff &lo = g->layers[l];
        const uint16_t *a16 = reinterpret_cast<const uint16_t *>(t->A[l]), *h16 = a16 + 4 * M * C;
        uint16_t *da16 = reinterpret_cast<uint16_t *>(t->DH);
        // MLP: DX = d x_out (its bf16 rounding is the gradient of the bf16 c_proj output)
        ep = tbk::Epi();
        ep.b16 = da16; ep.aux = a16; ep.ldc = 4 * C;
        if ((rc = bf_gemm<float, true, float, false, tbk::E_GELU_BWD>(t->DX, C, P + lo.proj2_w, 4 * C, M, 4 * C, C, ep, s)) != MGPT_OK) return rc;
        if ((rc = weight_grad_bf16(t, (const float *)t->DX, h16, G + lo.proj2_w, C, 4 * C, M, s)) != MGPT_OK) return rc;
        ep = tbk::Epi();
        ep.f32 = t->DXN; ep.ldc = C;
        if ((rc = bf_gemm<uint16_t, true, float, false, tbk::E_F32>(da16, 4 * C, P + lo.fc_w, C, M, C, 4 * C, ep, s)) != MGPT_OK) return rc;
        if ((rc = weight_grad_bf16(t, (const uint16_t *)da16, (const float *)t->XN2[l], G + lo.fc_w, 4 * C, C, M, s)) != MGPT_OK) return rc;
        if ((rc = ln_backward_bf16<true>(t, t->XM[l], P + lo.ln2, t->DXN, t->DX, G + lo.ln2, M, C, s)) != MGPT_OK) return rc;
        // attention: DX = d x_mid;  d y = bf16(DX W_proj), the gradient of the bf16 attention output
        const uint16_t *qkv16 = reinterpret_cast<const uint16_t *>(t->QKV[l]), *y16 = reinterpret_cast<const uint16_t *>(t->Y[l]);
        const float *ast = reinterpret_cast<const float *>(y16 + M * C);
        uint16_t *dy16 = reinterpret_cast<uint16_t *>(t->DY);
        ep = tbk::Epi();
        ep.b16 = dy16; ep.ldc = C;
        if ((rc = bf_gemm<float, true, float, false, tbk::E_B16>(t->DX, C, P + lo.proj_w, C, M, C, C, ep, s)) != MGPT_OK) return rc;
        if ((rc = weight_grad_bf16(t, (const float *)t->DX, y16, G + lo.proj_w, C, C, M, s)) != MGPT_OK) return rc;
        rc = g->hs == 32 ? attn_bwd_bf16<32>(t, qkv16, M * C, y16, dy16, ast, rows, g->nh, scale, s)
                         : attn_bwd_bf16<64>(t, qkv16, M * C, y16, dy16, ast, rows, g->nh, scale, s);
        if (rc != MGPT_OK) return rc;
        ep = tbk::Epi();
        ep.f32 = t->DXN; ep.ldc = C;
        if ((rc = bf_gemm<float, true, float, false, tbk::E_F32>(t->DQKV, 3 * C, P + lo.attn_w, C, M, C, 3 * C, ep, s)) != MGPT_OK) return rc;
        if ((rc = weight_grad_bf16(t, (const float *)t->DQKV, (const float *)t->XN1[l], G + lo.attn_w, 3 * C, C, M, s)) != MGPT_OK) return rc;
        if ((rc = ln_backward_bf16<true>(t, t->X[l], P + lo.ln1, t->DXN, t->DX, G + lo.ln1, M, C, s)) != MGPT_OK) return rc;
    }
    // embedding: the fp32 path's kernels
    hipLaunchKernelGGL(trk::wpe_bwd_kernel, dim3((unsigned)cdiv64((int64_t)kT * C, 256)), dim3(256), 0, s, (const float *)t->DX, rows, C, G + g->off_wpe);
    MGPT_LAUNCH_CHECK();
    {
        const int S = slabs_of(M), kps = slab_tokens(M);
        hipLaunchKernelGGL(trk::wte_bwd_part_kernel, dim3(kV, (unsigned)S), dim3(256), 0, s, tok, (const float *)t->DX, M, C, kps, t->part);
        MGPT_LAUNCH_CHECK();
        hipLaunchKernelGGL(trk::slab_reduce_kernel, dim3(grid_1d((int64_t)kV * C)), dim3(256), 0, s, t->part, S, (int64_t)kV * C, G + g->off_wte);
        MGPT_LAUNCH_CHECK();
    }
    return MGPT_OK;
}

int require_train(mgpt_gpt *g)
{
    MGPT_REQUIRE(g, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(g->train, MGPT_ERR_STATE, "no training workspace: mgpt_gpt_train_alloc first");
    return MGPT_OK;
}

}  // namespace

void gpt_train_destroy(mgpt_gpt *g)
{
    if (g->train) free_state(ts(g));
    g->train = nullptr;
}

extern "C" int mgpt_gpt_train_alloc(mgpt_gpt *g, int max_rows)
{
    MGPT_REQUIRE(g, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(max_rows > 0, MGPT_ERR_ARG, "max_rows=%d", max_rows);
    MGPT_REQUIRE(g->finalized, MGPT_ERR_STATE, "mgpt_gpt_finalize must precede mgpt_gpt_train_alloc");
    MGPT_REQUIRE(!g->has_bias, MGPT_ERR_UNSUPPORTED, "training supports bias = False checkpoints only (the released configs)");
    MGPT_REQUIRE(g->block == kT, MGPT_ERR_ARG, "training takes rows of T = 256 tokens; the model's block_size is %d", g->block);
    hipError_t e = hipSuccess;
    TrainState *t = ts(g);
    const bool fresh = t == nullptr;
    // an existing workspace keeps its gradients, AdamW moments and step counts: only the activation part is re-sized
    if (!fresh) {
        MGPT_HIP(hipDeviceSynchronize());              // (no queued call still uses the activations freed below)
        free_activations(t);
    } else {
        t = new TrainState();
    }
    auto alloc_in = [&](std::vector<void *> &owner, size_t bytes) -> void * {
        void *p = nullptr;
        if (e == hipSuccess) e = hipMalloc(&p, std::max<size_t>(bytes, 16));
        if (e == hipSuccess) owner.push_back(p);
        return e == hipSuccess ? p : nullptr;
    };
    const int64_t M = (int64_t)max_rows * kT, C = g->C;
    const int L = g->L;
    const size_t nt = 3 + 6 * (size_t)L;
    if (fresh) {
        auto fp = [&](int64_t n) { return static_cast<float *>(alloc_in(t->allocs, (size_t)n * sizeof(float))); };
        t->grads = fp(g->n_params); t->exp_avg = fp(g->n_params); t->exp_avg_sq = fp(g->n_params); t->steps = fp(nt);
        t->cnt = static_cast<int32_t *>(alloc_in(t->allocs, 2 * sizeof(int32_t)));
        t->loss_acc = static_cast<double *>(alloc_in(t->allocs, sizeof(double)));
        t->coef = fp(1);
        std::vector<trk::Blk> blk;
        const std::vector<TensorInfo> tt = tensor_table(g);
        for (size_t i = 0; i < tt.size(); i++)
            for (size_t b = 0; b < tt[i].count; b += trk::kChunk)
                blk.push_back({(int64_t)(tt[i].off + b), (int64_t)(tt[i].off + std::min(tt[i].count, b + trk::kChunk)), (int)i, tt[i].decay});
        t->n_blk = (int)blk.size();
        t->blk = static_cast<trk::Blk *>(alloc_in(t->allocs, blk.size() * sizeof(trk::Blk)));
        t->norm_part = static_cast<double *>(alloc_in(t->allocs, blk.size() * sizeof(double)));
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&t->h_cnt), 2 * sizeof(int32_t), hipHostMallocDefault);
        if (e == hipSuccess) e = hipMemcpy(t->blk, blk.data(), blk.size() * sizeof(trk::Blk), hipMemcpyHostToDevice);
        for (float *p : {t->grads, t->exp_avg, t->exp_avg_sq})
            if (e == hipSuccess) e = hipMemset(p, 0, g->n_params * sizeof(float));
        if (e == hipSuccess) e = hipMemset(t->steps, 0, nt * sizeof(float));
        if (e != hipSuccess) {
            set_error("training workspace allocation failed: %s", hipGetErrorString(e));
            free_state(t);
            return MGPT_ERR_HIP;
        }
        g->train = t;
    }
    auto fa = [&](int64_t n) { return static_cast<float *>(alloc_in(t->act_allocs, (size_t)n * sizeof(float))); };
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
    int rc = require_train(g);
    if (rc != MGPT_OK) return rc;
    MGPT_REQUIRE(d_tokens && d_targets, MGPT_ERR_ARG, "NULL argument");
    MGPT_REQUIRE(rows > 0, MGPT_ERR_ARG, "rows=%d", rows);
    MGPT_REQUIRE(T == kT, MGPT_ERR_ARG, "training takes rows of T = 256 tokens, got T = %d", T);
    MGPT_REQUIRE(!g->has_bias, MGPT_ERR_UNSUPPORTED, "training supports bias = False checkpoints only (the released configs)");
    MGPT_REQUIRE(precision == MGPT_PREC_F32 || precision == MGPT_PREC_BF16, MGPT_ERR_UNSUPPORTED,
                 "training precision %d: MGPT_PREC_F32 (exact fp32) or MGPT_PREC_BF16 (bf16 mixed precision)", precision);
    TrainState *t = ts(g);
    MGPT_REQUIRE(t->max_rows > 0, MGPT_ERR_STATE, "the training workspace holds no activation memory (a re-size failed): mgpt_gpt_train_alloc again");
    hipStream_t s = (hipStream_t)stream;
    // the cross-entropy normaliser is the targeted-position count of the WHOLE call (F.cross_entropy's mean over the call's tokens)
    hipLaunchKernelGGL(trk::count_targets_kernel, dim3(1), dim3(1024), 0, s, d_targets, (int64_t)rows * kT, t->cnt);
    MGPT_LAUNCH_CHECK();
    MGPT_HIP(hipMemcpyAsync(t->h_cnt, t->cnt, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MGPT_HIP(hipStreamSynchronize(s));
    MGPT_REQUIRE(t->h_cnt[1] == 0, MGPT_ERR_ARG, "targets must lie in [-1, 67): -1 is ignored, 0 .. 66 are vocabulary ids");
    MGPT_REQUIRE(t->h_cnt[0] > 0, MGPT_ERR_ARG, "no targeted position in the call (every target is -1): the mean cross-entropy is undefined");
    MGPT_HIP(hipMemsetAsync(t->loss_acc, 0, sizeof(double), s));
    for (int r0 = 0; r0 < rows; r0 += t->max_rows) {
        const int n = std::min(t->max_rows, rows - r0);
        const uint8_t *tk = d_tokens + (size_t)r0 * kT;
        const int32_t *tg = d_targets + (size_t)r0 * kT;
        rc = precision == MGPT_PREC_BF16 ? chunk_fwd_bwd_bf16(g, t, tk, n, tg, loss_scale, s) : chunk_fwd_bwd(g, t, tk, n, tg, loss_scale, s);
        if (rc != MGPT_OK) return rc;
    }
    if (d_loss) {
        hipLaunchKernelGGL(trk::loss_final_kernel, dim3(1), dim3(64), 0, s, (const double *)t->loss_acc, (const int32_t *)t->cnt, d_loss);
        MGPT_LAUNCH_CHECK();
    }
    return MGPT_OK;
}

extern "C" int mgpt_gpt_zero_grad(mgpt_gpt *g, void *stream)
{
    const int rc = require_train(g);
    if (rc != MGPT_OK) return rc;
    MGPT_HIP(hipMemsetAsync(ts(g)->grads, 0, g->n_params * sizeof(float), (hipStream_t)stream));
    return MGPT_OK;
}

extern "C" int mgpt_gpt_clip_grad_norm(mgpt_gpt *g, float max_norm, float *d_total_norm, void *stream)
{
    const int rc = require_train(g);
    if (rc != MGPT_OK) return rc;
    TrainState *t = ts(g);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(trk::sumsq_part_kernel, dim3((unsigned)t->n_blk), dim3(256), 0, s, (const float *)t->grads, (const trk::Blk *)t->blk, t->norm_part);
    MGPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(trk::clip_coef_kernel, dim3(1), dim3(64), 0, s, (const double *)t->norm_part, (const trk::Blk *)t->blk, t->n_blk,
                       max_norm > 0.f ? max_norm : 1.f, d_total_norm, t->coef);
    MGPT_LAUNCH_CHECK();
    if (max_norm > 0.f) {
        hipLaunchKernelGGL(trk::scale_kernel, dim3(grid_1d((int64_t)g->n_params)), dim3(256), 0, s, t->grads, (int64_t)g->n_params, (const float *)t->coef);
        MGPT_LAUNCH_CHECK();
    }
    return MGPT_OK;
}

extern "C" int mgpt_gpt_adamw_step(mgpt_gpt *g, float lr, float beta1, float beta2, float eps, float weight_decay, void *stream)
{
    const int rc = require_train(g);
    if (rc != MGPT_OK) return rc;
    MGPT_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && lr >= 0.f, MGPT_ERR_ARG,
                 "AdamW hyper-parameters out of range (lr %g, betas %g %g, eps %g)", lr, beta1, beta2, eps);
    TrainState *t = ts(g);
    hipStream_t s = (hipStream_t)stream;
    const int nt = 3 + 6 * g->L;
    hipLaunchKernelGGL(trk::step_inc_kernel, dim3((unsigned)cdiv(nt, 256)), dim3(256), 0, s, t->steps, nt);
    MGPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(trk::adamw_kernel, dim3((unsigned)t->n_blk), dim3(256), 0, s, g->params, (const float *)t->grads, t->exp_avg, t->exp_avg_sq,
                       (const trk::Blk *)t->blk, (const float *)t->steps, lr, beta1, beta2, eps, weight_decay);
    MGPT_LAUNCH_CHECK();
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
    int rc = MGPT_OK;
    MGPT_REQUIRE(g && d_out, MGPT_ERR_ARG, "NULL argument");
    float *src = nullptr;
    size_t count = 0;
    if ((rc = train_locate(g, name, which, &src, &count)) != MGPT_OK) return rc;
    MGPT_REQUIRE((size_t)n_elem == count, MGPT_ERR_ARG, "'%s' (which %d): got %lld elements, expected %zu", name, which, (long long)n_elem, count);
    MGPT_HIP(hipMemcpyAsync(d_out, src, count * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MGPT_OK;
}

extern "C" int mgpt_gpt_train_set(mgpt_gpt *g, const char *name, int which, const float *data, int64_t n_elem, int is_device)
{
    int rc = MGPT_OK;
    MGPT_REQUIRE(g && data, MGPT_ERR_ARG, "NULL argument");
    float *dst = nullptr;
    size_t count = 0;
    if ((rc = train_locate(g, name, which, &dst, &count)) != MGPT_OK) return rc;
    MGPT_REQUIRE((size_t)n_elem == count, MGPT_ERR_ARG, "'%s' (which %d): got %lld elements, expected %zu", name, which, (long long)n_elem, count);
    MGPT_HIP(hipDeviceSynchronize());                  // (stream-ordered work on the tensor finishes first: this call is synchronous)
    MGPT_HIP(hipMemcpy(dst, data, count * sizeof(float), is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    if (which == MGPT_TRAIN_PARAM) gpt_params_changed(g);
    return MGPT_OK;
}
