// gpt_kernels_train.h -- exact-fp32 backward, gradient clipping and AdamW kernels (mgpt_gpt_forward_backward & co., train.hip), gfx950.
//
// Training is what train.py:324-331 does: bias = False, rows of T = 256 tokens, dropout by counter-hash masks (Drop below).  The forward that
// saves activations runs the exact-fp32 forward kernels of gpt_kernels_f32.h (gemm_f32_kernel, attn_f32_kernel, layernorm_kernel); the
// kernels here are the backward and the optimizer.  Every product is an fp32 fmaf on the VALU, every reduction runs in a fixed order and
// no kernel uses a floating-point atomic: two identical calls give bit-identical gradients.
//
// Layouts (M = rows * 256 tokens of one workspace chunk):
//   token-major [M][N] activations and gradients (x, ln outputs, y, c_fc pre-activation, dY, dq|dk|dv as [M][3C]);
//   q, k, v head-major [rows][n_head][256][hs] planes, as the forward's EPI_QKV epilogue writes them;
//   weight-gradient partials [S][N][K]: slab s sums the tokens [s * kps, (s + 1) * kps), slab_reduce_kernel adds the slabs in order.
#pragma once
#include "common.h"

namespace mgpt {
namespace trk {

constexpr int kT = 256;

// ----- strided GEMM: C(m, n) (op)= sum_{k in the split's range} A(m, k) * B(k, n), 64 x 64 tiles, 4 x 4 outputs per thread -----
// A(m, k) = A[m * lda + k] (A_KC) or A[k * lda + m];  B(k, n) = B[k * ldb + n] (B_NC) or B[n * ldb + k].  Every index is bounds-checked,
// so any M, N, K work.  k runs in increasing order: an fmaf chain over each 16-wide k tile, the tiles' sums added in order (a long chain
// of K fmafs would grow the rounding error with K: the c_attn input gradient of 85M sums 2304 terms).
enum { OUT_STORE = 0, OUT_RESID = 1, OUT_PART = 2, OUT_GELU_BWD = 3 };     // (the values are part of the instances' symbol names)

__device__ __forceinline__ float gelu_grad(float a)
{
    // d/da [0.5 a (1 + erf(a / sqrt 2))] = 0.5 (1 + erf(a / sqrt 2)) + a * exp(-a^2 / 2) / sqrt(2 pi)
    return 0.5f * (1.0f + erff(a * 0.70710678118654752440f)) + a * expf(-0.5f * a * a) * 0.39894228040143267794f;
}

template <bool A_KC, bool B_NC, int OUT>
__global__ __launch_bounds__(256) void gemm_tr_kernel(const float *__restrict__ A, int64_t lda, const float *__restrict__ B, int64_t ldb,
                                                      float *__restrict__ Cout, int64_t ldc, int M, int N, int K, int kps,
                                                      const float *__restrict__ aux)
{
    constexpr int BM = 64, BN = 64, BK = 16;
    __shared__ __attribute__((aligned(16))) float sA[BK][BM];
    __shared__ __attribute__((aligned(16))) float sB[BK][BN];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
    const int kb = blockIdx.z * kps, ke = min(K, kb + kps);
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.f;
    for (int k0 = kb; k0 < ke; k0 += BK) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int idx = tid + 256 * e;
            int mm, kk;
            if (A_KC) { mm = idx >> 4; kk = idx & 15; } else { mm = idx & 63; kk = idx >> 6; }
            const int m = m0 + mm, k = k0 + kk;
            sA[kk][mm] = (m < M && k < ke) ? (A_KC ? A[(int64_t)m * lda + k] : A[(int64_t)k * lda + m]) : 0.f;
            int nn, kn;
            if (B_NC) { nn = idx & 63; kn = idx >> 6; } else { nn = idx >> 4; kn = idx & 15; }
            const int n = n0 + nn, k2 = k0 + kn;
            sB[kn][nn] = (n < N && k2 < ke) ? (B_NC ? B[(int64_t)k2 * ldb + n] : B[(int64_t)n * ldb + k2]) : 0.f;
        }
        __syncthreads();
        float tile[4][4];                                       // this k tile's 16 products per output, then added: two-level summation
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) tile[i][j] = 0.f;
#pragma unroll
        for (int kk = 0; kk < BK; kk++) {
            const float4 a = *reinterpret_cast<const float4 *>(&sA[kk][ty * 4]);
            const float4 b = *reinterpret_cast<const float4 *>(&sB[kk][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) tile[i][j] = fmaf(av[i], bv[j], tile[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] += tile[i][j];
        __syncthreads();
    }
    float *dst = OUT == OUT_PART ? Cout + (int64_t)blockIdx.z * M * ldc : Cout;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int m = m0 + ty * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int n = n0 + tx * 4 + j;
            if (n >= N) continue;
            const int64_t o = (int64_t)m * ldc + n;
            if (OUT == OUT_GELU_BWD) dst[o] = acc[i][j] * gelu_grad(aux[o]);
            else if (OUT == OUT_RESID) dst[o] = aux[o] + acc[i][j];     // a residual branch joins the stream aux (the compact last layer)
            else dst[o] = acc[i][j];
        }
    }
}

// ----- dropout (model.py:33-34, 59, 66, 71, 82, 88, 129, 175; restated in mapf_gpt_amd/sampling.py: dropout_keep) -----
// A mask is a pure function of (seed, step, site, layer, element index): forward and backward regenerate it and nothing is stored.  Sites:
// 0 the embedding sum, 1 the attention probabilities, 2 attention's residual branch, 3 the MLP's.  Element index of site 1:
// ((row0 + row) * n_head + head) * 65536 + query * 256 + key; of the others ((row0 + row) * 256 + t) * C + c; row counts from the start of
// the CALL, so a mask does not depend on the workspace's chunking.  One splitmix64 value serves four consecutive elements: element e takes
// bits 16 (e & 3) of hash(e >> 2), is kept iff they are >= thr = round(p * 65536), and kept values are scaled by 1 / (1 - thr / 65536).
struct Drop {
    uint64_t key = 0;       // drop_key(seed, step, site, layer), computed on the host
    uint64_t base = 0;      // element index of the chunk's first element
    uint32_t thr = 0;
    float scale = 1.f;
};

__host__ __device__ __forceinline__ uint64_t drop_fmix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the stream's key: the sampler's (seed, step) word (gpt.hip: uniform01) with the stream id folded in, finalised
inline uint64_t drop_key(uint64_t seed, uint64_t step, int site, int layer)
{
    return drop_fmix((seed + 0x9E3779B97F4A7C15ull * (step + 1ull)) ^ ((uint64_t)(site * 256 + layer + 1) * 0xD1342543DE82EF95ull));
}
// the 64 mask bits of the elements 4 e4 .. 4 e4 + 3
__device__ __forceinline__ uint64_t drop_hash(uint64_t key, uint64_t e4) { return drop_fmix(key + 0x9E3779B97F4A7C15ull * (e4 + 1ull)); }
// ... as hash(b4 + l) with a wave-uniform b4: kb = drop_base(key, b4) on the scalar unit once, then a 64 x 32-bit product per hash
__device__ __forceinline__ uint64_t drop_base(uint64_t key, uint64_t b4) { return key + 0x9E3779B97F4A7C15ull * (b4 + 1ull); }
__device__ __forceinline__ uint64_t drop_hash_at(uint64_t kb, uint32_t l) { return drop_fmix(kb + 0x9E3779B97F4A7C15ull * (uint64_t)l); }
__device__ __forceinline__ bool drop_keep(uint64_t h, int slot, uint32_t thr) { return ((uint32_t)(h >> (16 * slot)) & 0xffffu) >= thr; }
// the factor of element `slot` of the hash: scale if kept, 0 if dropped
__device__ __forceinline__ float drop_factor(uint64_t h, int slot, const Drop &d) { return drop_keep(h, slot, d.thr) ? d.scale : 0.f; }

// out[i] = m s v(in[i]) over n4 quads of elements (the quad index is the hash's counter: base and n are multiples of 4);  v rounds to bf16
// first when ROUND (the bf16 path's gradient of a bf16 branch output).  in == out is allowed.
template <bool ROUND>
__global__ __launch_bounds__(256) void drop_scale_kernel(const float *in, float *out, int64_t n4, Drop d)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const uint64_t h = drop_hash(d.key, (d.base >> 2) + (uint64_t)i);
        float4 v = reinterpret_cast<const float4 *>(in)[i];
        if (ROUND) { v.x = (float)(__bf16)v.x; v.y = (float)(__bf16)v.y; v.z = (float)(__bf16)v.z; v.w = (float)(__bf16)v.w; }    // (nearest-even)
        reinterpret_cast<float4 *>(out)[i] =
            make_float4(v.x * drop_factor(h, 0, d), v.y * drop_factor(h, 1, d), v.z * drop_factor(h, 2, d), v.w * drop_factor(h, 3, d));
    }
}

// out[i] = x[i] + m s o[i]: a residual branch's output o joins the stream (fp32 path)
__global__ __launch_bounds__(256) void drop_resid_kernel(const float *__restrict__ x, const float *__restrict__ o, float *__restrict__ out,
                                                         int64_t n4, Drop d)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const uint64_t h = drop_hash(d.key, (d.base >> 2) + (uint64_t)i);
        const float4 r = reinterpret_cast<const float4 *>(x)[i], v = reinterpret_cast<const float4 *>(o)[i];
        reinterpret_cast<float4 *>(out)[i] = make_float4(r.x + v.x * drop_factor(h, 0, d), r.y + v.y * drop_factor(h, 1, d),
                                                         r.z + v.z * drop_factor(h, 2, d), r.w + v.w * drop_factor(h, 3, d));
    }
}

// out[i] += sum_{s < S} part[s * n + i], s in increasing order
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float *__restrict__ part, int S, int64_t n, float *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float s = 0.f;
        for (int k = 0; k < S; k++) s += part[(int64_t)k * n + i];
        out[i] += s;
    }
}

// out[i] = scale * (((g[0][i] + g[1][i]) + g[2][i]) + ...), g = gathered [world][n]: the ranks' gradient buffers added in rank order with
// plain fp32 additions, then one multiplication (train.py:237-239: DDP's mean over the ranks, here in an order the code fixes, so every
// rank computes the same bits).  out is REPLACED.  Bandwidth-bound ((world + 1) * 4 n bytes): the first nv = n / 4 quads move as 16-byte
// loads and stores -- the caller passes nv > 0 only when gathered, out and every row g[r] = gathered + r * n are 16-byte aligned
// (n % 4 == 0) -- and the elements from 4 nv on one by one.
__global__ __launch_bounds__(256) void rank_reduce_kernel(const float *__restrict__ gathered, int world, int64_t n, int64_t nv, float scale,
                                                          float *__restrict__ out)
{
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const float4 *g4 = reinterpret_cast<const float4 *>(gathered);
    float4 *o4 = reinterpret_cast<float4 *>(out);
    const int64_t row4 = n / 4;                                 // (quads per row; read only when nv > 0, i.e. n % 4 == 0)
    for (int64_t i = t0; i < nv; i += stride) {
        float4 s = g4[i];
#pragma unroll 4
        for (int r = 1; r < world; r++) {
            const float4 v = g4[(int64_t)r * row4 + i];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        o4[i] = make_float4(s.x * scale, s.y * scale, s.z * scale, s.w * scale);
    }
    for (int64_t i = 4 * nv + t0; i < n; i += stride) {
        float s = gathered[i];
        for (int r = 1; r < world; r++) s += gathered[(int64_t)r * n + i];
        out[i] = s * scale;
    }
}

// part[s][c] = sum over the tokens of slab s of v[m][c] (LayerNorm gain gradients), m in increasing order, accumulated in double
__global__ __launch_bounds__(256) void colsum_part_kernel(const float *__restrict__ v, int64_t M, int C, int kps, float *__restrict__ part)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t mb = (int64_t)blockIdx.y * kps, me = min<int64_t>(M, mb + kps);
    double s = 0.0;                                             // (a column sum of fp32 terms, kept in double)
    for (int64_t m = mb; m < me; m++) s += (double)v[m * C + c];
    part[(int64_t)blockIdx.y * C + c] = (float)s;
}

__global__ __launch_bounds__(256) void gelu_kernel(const float *__restrict__ a, float *__restrict__ h, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = a[i];
        h[i] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));     // = f32k::gelu_erf
    }
}

// ----- LayerNorm backward (eps 1e-5, gain only), one wavefront per token -----
// dres[m] (+)= rstd * (g - mean(g) - xhat * mean(g * xhat)) with g = dxn * w;  gp[m] = dxn * xhat (the gain's per-token terms)
template <bool ADD>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ dxn,
                                                     float *__restrict__ dres, float *__restrict__ gp, int64_t n_tok, int C)
{
    const int lane = threadIdx.x & 63;
    const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= n_tok) return;
    const float *px = x + tok * C, *pd = dxn + tok * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += px[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = px[c] - mean; q = fmaf(d, d, q); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)C + 1e-5f);
    float sg = 0.f, sgx = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float xh = (px[c] - mean) * rstd, g = pd[c] * w[c];
        sg += g;
        sgx = fmaf(g, xh, sgx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sg += __shfl_xor(sg, o); sgx += __shfl_xor(sgx, o); }
    const float mg = sg / (float)C, mgx = sgx / (float)C;
    for (int c = lane; c < C; c += 64) {
        const float xh = (px[c] - mean) * rstd, g = pd[c] * w[c];
        const float dx = rstd * (g - mg - xh * mgx);
        if (ADD) dres[tok * C + c] += dx; else dres[tok * C + c] = dx;
        gp[tok * C + c] = pd[c] * xh;
    }
}

// ----- cross-entropy (ignore_index = -1) on every token: dlogits = (softmax - onehot) * scale / count, nll per token -----
__global__ __launch_bounds__(256) void ce_kernel(const float *__restrict__ logits, const int32_t *__restrict__ targets, int64_t M,
                                                 const int32_t *__restrict__ d_count, float loss_scale, float *__restrict__ dlogits,
                                                 float *__restrict__ tok_nll)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int tg = targets[m];
    const float *l = logits + m * MGPT_VOCAB;
    float *dl = dlogits + m * MGPT_VOCAB;
    if (tg < 0 || tg >= MGPT_VOCAB) {
        for (int v = 0; v < MGPT_VOCAB; v++) dl[v] = 0.f;
        tok_nll[m] = 0.f;
        return;
    }
    float mx = l[0];
    for (int v = 1; v < MGPT_VOCAB; v++) mx = fmaxf(mx, l[v]);
    float sum = 0.f;
    for (int v = 0; v < MGPT_VOCAB; v++) sum += expf(l[v] - mx);
    const float lse = mx + logf(sum);
    const float k = loss_scale / (float)(*d_count);
    for (int v = 0; v < MGPT_VOCAB; v++) {
        const float p = expf(l[v] - lse);
        dl[v] = (p - (v == tg ? 1.f : 0.f)) * k;
    }
    tok_nll[m] = lse - l[tg];
}

// targeted positions of a whole call (0 <= t < 67) into cnt[0]; cnt[1] = 1 if any target is outside [-1, 67).  One workgroup.
__global__ __launch_bounds__(1024) void count_targets_kernel(const int32_t *__restrict__ t, int64_t n, int32_t *__restrict__ cnt)
{
    __shared__ int sc[1024], sb[1024];
    int c = 0, bad = 0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const int v = t[i];
        c += (v >= 0 && v < MGPT_VOCAB);
        bad |= (v < -1 || v >= MGPT_VOCAB);
    }
    sc[threadIdx.x] = c; sb[threadIdx.x] = bad;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sc[threadIdx.x] += sc[threadIdx.x + o]; sb[threadIdx.x] |= sb[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { cnt[0] = sc[0]; cnt[1] = sb[0]; }
}

// acc[0] += sum of v[0 .. n) (double, fixed tree order); one workgroup, stream-ordered across chunks
__global__ __launch_bounds__(256) void sum_acc_kernel(const float *__restrict__ v, int64_t n, double *__restrict__ acc)
{
    __shared__ double sd[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)v[i];
    sd[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sd[threadIdx.x] += sd[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) acc[0] += sd[0];
}

__global__ void loss_final_kernel(const double *__restrict__ acc, const int32_t *__restrict__ cnt, float *__restrict__ loss)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) loss[0] = (float)(acc[0] / (double)cnt[0]);
}

// ----- attention backward (model.py:58-60, non-causal, T = 256), one workgroup per (row, head), thread = query / key -----
// P is recomputed from q, k: s = (q . k) * scale, P = exp(s - m) / l with the query's (m, l) from attn_bwd_q_kernel; D = rowsum(dY o Y).
// dQ = dS K * scale (this kernel, also stores (m, l, D) per query), dV = P^T dY and dK = dS^T Q * scale (attn_bwd_kv_kernel).
template <int HS>
__device__ __forceinline__ float dot_lds(const float *a, const float *__restrict__ b)
{
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HS; d += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(b + d);
        s = fmaf(a[d], v.x, s); s = fmaf(a[d + 1], v.y, s); s = fmaf(a[d + 2], v.z, s); s = fmaf(a[d + 3], v.w, s);
    }
    return s;
}

// dynamic LDS of the two kernels below: K and V (q), or Q, dY and three statistics per query (kv), of one (row, head)
template <int HS>
constexpr size_t attn_bwd_q_lds() { return (size_t)2 * kT * HS * sizeof(float); }
template <int HS>
constexpr size_t attn_bwd_kv_lds() { return attn_bwd_q_lds<HS>() + (size_t)3 * kT * sizeof(float); }

// DROP (dropout on P, site 1): y = sum_j m s P v, so dP = m s (dy . v) and dV takes m s P; D = rowsum(dY o Y) holds for the dropped y, and
// the statistics (m, l) run over all keys
template <int HS, bool DROP = false>
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const float *__restrict__ qkv, int64_t plane, const float *__restrict__ Y,
                                                         const float *__restrict__ dY, float *__restrict__ dqkv, float *__restrict__ stats,
                                                         int n_head, float scale, Drop dr)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sK = smem, *sV = smem + kT * HS;
    const int bh = blockIdx.x, b = bh / n_head, head = bh - b * n_head, C = n_head * HS;
    const float *Q = qkv + (int64_t)bh * kT * HS, *K = Q + plane, *V = Q + 2 * plane;
    for (int i = threadIdx.x; i < kT * HS / 4; i += 256) {
        reinterpret_cast<float4 *>(sK)[i] = reinterpret_cast<const float4 *>(K)[i];
        reinterpret_cast<float4 *>(sV)[i] = reinterpret_cast<const float4 *>(V)[i];
    }
    __syncthreads();
    const int i = threadIdx.x;
    const int64_t tok = (int64_t)b * kT + i;
    float q[HS], dy[HS], acc[HS];
    float D = 0.f;
#pragma unroll
    for (int d = 0; d < HS; d++) {
        q[d] = Q[i * HS + d];
        dy[d] = dY[tok * C + head * HS + d];
        D = fmaf(dy[d], Y[tok * C + head * HS + d], D);
        acc[d] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < kT; j++) {
        const float s = dot_lds<HS>(q, sK + j * HS) * scale;
        if (s > m) { l = l * expf(m - s) + 1.f; m = s; }
        else l += expf(s - m);
    }
    const float inv_l = 1.f / l;
    [[maybe_unused]] uint64_t kb = 0, h = 0;                    // (DROP) the base of this (row, head)'s 65536 elements, four keys' hash
    if constexpr (DROP) kb = drop_base(dr.key, (dr.base >> 2) + (uint64_t)bh * (kT * kT / 4));
    for (int j = 0; j < kT; j++) {
        const float s = dot_lds<HS>(q, sK + j * HS) * scale;
        const float p = expf(s - m) * inv_l;
        float ds;
        if constexpr (DROP) {
            if ((j & 3) == 0) h = drop_hash_at(kb, (uint32_t)(i * kT + j) >> 2);
            ds = p * (dot_lds<HS>(dy, sV + j * HS) * drop_factor(h, j & 3, dr) - D);
        } else {
            ds = p * (dot_lds<HS>(dy, sV + j * HS) - D);
        }
        const float *kr = sK + j * HS;
#pragma unroll
        for (int d = 0; d < HS; d++) acc[d] = fmaf(ds, kr[d], acc[d]);
    }
    float *o = dqkv + tok * 3 * C + head * HS;
#pragma unroll
    for (int d = 0; d < HS; d++) o[d] = acc[d] * scale;
    float *st = stats + ((int64_t)bh * kT + i) * 3;
    st[0] = m; st[1] = inv_l; st[2] = D;
}

// MODE 0: dV (thread = key j: sum_i P_ij dY_i);  MODE 1: dK (sum_i dS_ij Q_i * scale)
template <int HS, int MODE, bool DROP = false>
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const float *__restrict__ qkv, int64_t plane, const float *__restrict__ dY,
                                                          float *__restrict__ dqkv, const float *__restrict__ stats, int n_head, float scale,
                                                          Drop dp)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sQ = smem, *sD = smem + kT * HS, *sS = smem + 2 * kT * HS;
    const int bh = blockIdx.x, b = bh / n_head, head = bh - b * n_head, C = n_head * HS;
    const float *Q = qkv + (int64_t)bh * kT * HS, *K = Q + plane, *V = Q + 2 * plane;
    for (int i = threadIdx.x; i < kT * HS / 4; i += 256) {
        reinterpret_cast<float4 *>(sQ)[i] = reinterpret_cast<const float4 *>(Q)[i];
        const int t = (4 * i) / HS, d = 4 * i - t * HS;
        reinterpret_cast<float4 *>(sD)[i] = *reinterpret_cast<const float4 *>(dY + ((int64_t)b * kT + t) * C + head * HS + d);
    }
    for (int i = threadIdx.x; i < kT * 3; i += 256) sS[i] = stats[(int64_t)bh * kT * 3 + i];
    __syncthreads();
    const int j = threadIdx.x;
    float k[HS], v[MODE == 1 ? HS : 1], acc[HS];
#pragma unroll
    for (int d = 0; d < HS; d++) {
        k[d] = K[j * HS + d];
        if constexpr (MODE == 1) v[d] = V[j * HS + d];
        acc[d] = 0.f;
    }
    for (int i = 0; i < kT; i++) {
        // the same fmaf chain as attn_bwd_q_kernel's s (q . k over d in order): P is bit-identical in both kernels
        const float *qr = sQ + i * HS;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < HS; d += 4) {
            const float4 a = *reinterpret_cast<const float4 *>(qr + d);
            s = fmaf(a.x, k[d], s); s = fmaf(a.y, k[d + 1], s); s = fmaf(a.z, k[d + 2], s); s = fmaf(a.w, k[d + 3], s);
        }
        const float p = expf(s * scale - sS[3 * i]) * sS[3 * i + 1];
        const float *dr = sD + i * HS;
        float f = 1.f;                                          // (DROP) m s of (query i, key j)
        if constexpr (DROP)
            f = drop_factor(drop_hash_at(drop_base(dp.key, (dp.base >> 2) + (uint64_t)bh * (kT * kT / 4)), (uint32_t)(i * kT + j) >> 2), j & 3, dp);
        if constexpr (MODE == 0 && DROP) {
            const float pm = p * f;
#pragma unroll
            for (int d = 0; d < HS; d++) acc[d] = fmaf(pm, dr[d], acc[d]);
        } else if constexpr (MODE == 0) {
#pragma unroll
            for (int d = 0; d < HS; d++) acc[d] = fmaf(p, dr[d], acc[d]);
        } else if constexpr (DROP) {
            const float ds = p * (dot_lds<HS>(v, dr) * f - sS[3 * i + 2]);
#pragma unroll
            for (int d = 0; d < HS; d++) acc[d] = fmaf(ds, qr[d], acc[d]);
        } else {
            const float ds = p * (dot_lds<HS>(v, dr) - sS[3 * i + 2]);
#pragma unroll
            for (int d = 0; d < HS; d++) acc[d] = fmaf(ds, qr[d], acc[d]);
        }
    }
    float *o = dqkv + ((int64_t)b * kT + j) * 3 * C + (MODE == 0 ? 2 : 1) * C + head * HS;
#pragma unroll
    for (int d = 0; d < HS; d++) o[d] = MODE == 0 ? acc[d] : acc[d] * scale;
}

// ----- attention forward with dropout on P (fp32 path): f32k::attn_f32_kernel's walk for T = 256 (S^T = K Q^T per 32-query tile on
// v_mfma_f32_32x32x2f32, keys in tiles of 32 with a running (max, sum)), the mask applied to exp(s - max) AFTER it joined the sum: the
// softmax sum runs over all keys, y = s / l * sum_j m_j p_j v_j -----
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int HS>
__global__ __launch_bounds__(256) void attn_fwd_drop_kernel(const float *__restrict__ qkv, int64_t plane, float *__restrict__ y, int n_head,
                                                            float scale, Drop dp)
{
    constexpr int HH = HS / 2, DT = HS / 32, KT = kT / 32;
    const int bh = blockIdx.x, b = bh / n_head, head = bh - b * n_head, C = n_head * HS;
    const float *Q = qkv + (int64_t)bh * kT * HS, *Kp = Q + plane, *V = Q + 2 * plane;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    for (int qt = wave; qt < KT; qt += 4) {
        float4 qf[HH / 4];
#pragma unroll
        for (int i = 0; i < HH / 4; i++) qf[i] = *reinterpret_cast<const float4 *>(Q + (qt * 32 + r) * HS + h * HH + 4 * i);
        f32x16 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; dt++)
#pragma unroll
            for (int g = 0; g < 16; g++) o[dt][g] = 0.f;
        float m_run = -INFINITY, l_run = 0.f;
        const uint64_t kb = drop_base(dp.key, (dp.base >> 2) + (uint64_t)bh * (kT * kT / 4));
        const uint32_t e0 = (uint32_t)(qt * 32 + r) * kT;       // the query's first element within this (row, head)
#pragma unroll 1
        for (int kt = 0; kt < KT; kt++) {
            f32x16 s;
#pragma unroll
            for (int g = 0; g < 16; g++) s[g] = 0.f;
            const float *krow = Kp + (kt * 32 + r) * HS + h * HH;
#pragma unroll
            for (int i = 0; i < HH / 4; i++) {
                const float4 kf = *reinterpret_cast<const float4 *>(krow + 4 * i);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[i].x, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[i].y, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[i].z, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[i].w, s, 0, 0, 0);
            }
            // s[g] = S[query r][key = kt * 32 + (g & 3) + 8 * (g >> 2) + 4 * h]
            float mx = s[0];
#pragma unroll
            for (int g = 1; g < 16; g++) mx = fmaxf(mx, s[g]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = expf((m_run - m_new) * scale);
            float psum = 0.f;
#pragma unroll
            for (int g = 0; g < 16; g++) {
                s[g] = expf((s[g] - m_new) * scale);
                psum += s[g];
            }
            psum += __shfl_xor(psum, 32);
            l_run = l_run * alpha + psum;
            m_run = m_new;
#pragma unroll
            for (int gg = 0; gg < 4; gg++) {                    // four consecutive keys kt * 32 + 8 gg + 4 h ..: one hash
                const uint64_t hh = drop_hash_at(kb, (e0 + kt * 32 + 8 * gg + 4 * h) >> 2);
#pragma unroll
                for (int i = 0; i < 4; i++) s[4 * gg + i] = drop_keep(hh, i, dp.thr) ? s[4 * gg + i] : 0.f;
            }
#pragma unroll
            for (int dt = 0; dt < DT; dt++)
#pragma unroll
                for (int g = 0; g < 16; g++) o[dt][g] *= alpha;
            const float *vbase = V + (kt * 32 + 4 * h) * HS + r;
#pragma unroll
            for (int g = 0; g < 16; g++) {
                const int key = (g & 3) + 8 * (g >> 2);
#pragma unroll
                for (int dt = 0; dt < DT; dt++) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vbase[key * HS + dt * 32], s[g], o[dt], 0, 0, 0);
            }
        }
        const float inv = dp.scale / l_run;
        // o[dt][g] = O[query r][d = dt * 32 + (g & 3) + 8 * (g >> 2) + 4 * h]
        float *yrow = y + ((int64_t)b * kT + qt * 32 + r) * C + head * HS;
#pragma unroll
        for (int dt = 0; dt < DT; dt++)
#pragma unroll
            for (int gg = 0; gg < 4; gg++)
                *reinterpret_cast<float4 *>(yrow + dt * 32 + 8 * gg + 4 * h) =
                    make_float4(o[dt][4 * gg] * inv, o[dt][4 * gg + 1] * inv, o[dt][4 * gg + 2] * inv, o[dt][4 * gg + 3] * inv);
    }
}

// ===== the last-position micro-step (mgpt_gpt_forward_backward_rows): one targeted position per row, token 255 =====
// The last layer runs its attention output, out-projection, MLP, ln_f, head and cross-entropy on a compact matrix [mc][C] of the rows'
// last tokens (row r of the chunk = token r * 256 + 255); rows >= n_rows of the compact matrix are zero padding (the bf16 GEMMs take
// token counts in multiples of 32), and zero rows stay zero through every step.

// dst[r][c] = src[(r * 256 + 255)][c] for r < n_rows, 0 for the padding rows up to mc
__global__ __launch_bounds__(256) void gather_last_kernel(const float *__restrict__ src, float *__restrict__ dst, int n_rows, int mc, int C)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)mc * C; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / C), c = (int)(i - (int64_t)r * C);
        dst[i] = r < n_rows ? src[((int64_t)r * kT + kT - 1) * C + c] : 0.f;
    }
}

// dst[(r * 256 + 255)][c] += src[r][c], r < n_rows: a compact gradient joins the dense one (every element has one writer)
__global__ __launch_bounds__(256) void scatter_last_add_kernel(const float *__restrict__ src, float *__restrict__ dst, int n_rows, int C)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)n_rows * C; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / C), c = (int)(i - (int64_t)r * C);
        dst[((int64_t)r * kT + kT - 1) * C + c] += src[i];
    }
}

// The two residual joins of the compact matrix under dropout (sites 2 and 3): compact row r is token 255 of row r, so its mask elements are
// ((row0 + r) * 256 + 255) * C + c -- the mask's row pitch is 256 C while the data's is C.  d.base = the element of compact row 0, column 0;
// a quad index is the hash's counter (C a multiple of 4).
__device__ __forceinline__ uint64_t drop_last_hash(const Drop &d, int64_t i, int C4)
{
    const int64_t r = i / C4;
    return drop_hash(d.key, (d.base >> 2) + (uint64_t)r * (uint64_t)(kT * C4) + (uint64_t)(i - r * C4));
}

// out[r][c] = x[r][c] + m s o[r][c] over n_rows compact rows (fp32 path)
__global__ __launch_bounds__(256) void drop_resid_last_kernel(const float *__restrict__ x, const float *__restrict__ o, float *__restrict__ out,
                                                              int n_rows, int C, Drop d)
{
    const int C4 = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)n_rows * C4; i += (int64_t)gridDim.x * 256) {
        const uint64_t h = drop_last_hash(d, i, C4);
        const float4 r = reinterpret_cast<const float4 *>(x)[i], v = reinterpret_cast<const float4 *>(o)[i];
        reinterpret_cast<float4 *>(out)[i] = make_float4(r.x + v.x * drop_factor(h, 0, d), r.y + v.y * drop_factor(h, 1, d),
                                                         r.z + v.z * drop_factor(h, 2, d), r.w + v.w * drop_factor(h, 3, d));
    }
}

// out[r][c] = m s v(in[r][c]): the gradient that enters a compact residual branch's c_proj;  v rounds to bf16 first when ROUND
template <bool ROUND>
__global__ __launch_bounds__(256) void drop_scale_last_kernel(const float *__restrict__ in, float *__restrict__ out, int n_rows, int C, Drop d)
{
    const int C4 = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)n_rows * C4; i += (int64_t)gridDim.x * 256) {
        const uint64_t h = drop_last_hash(d, i, C4);
        float4 v = reinterpret_cast<const float4 *>(in)[i];
        if (ROUND) { v.x = (float)(__bf16)v.x; v.y = (float)(__bf16)v.y; v.z = (float)(__bf16)v.z; v.w = (float)(__bf16)v.w; }    // (nearest-even)
        reinterpret_cast<float4 *>(out)[i] =
            make_float4(v.x * drop_factor(h, 0, d), v.y * drop_factor(h, 1, d), v.z * drop_factor(h, 2, d), v.w * drop_factor(h, 3, d));
    }
}

// cross-entropy of the compact logits [mc][67] against one label per row; k = loss_scale / rows of the WHOLE call, a host-side number (no
// count is read from the device).  The label is compared with [0, 67) before anything is indexed with it: an out-of-range label makes the
// row's loss term and its dlogits NaN -- the call's loss and the next gradient norm are NaN, loudly, and no host wait is spent on it.
__global__ __launch_bounds__(256) void ce_rows_kernel(const float *__restrict__ logits, const int32_t *__restrict__ labels, int n_rows, int mc,
                                                      float k, float *__restrict__ dlogits, float *__restrict__ row_nll)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= mc) return;
    float *dl = dlogits + (int64_t)r * MGPT_VOCAB;
    if (r >= n_rows) {
        for (int v = 0; v < MGPT_VOCAB; v++) dl[v] = 0.f;
        row_nll[r] = 0.f;
        return;
    }
    const int tg = labels[r];
    if (tg < 0 || tg >= MGPT_VOCAB) {
        const float nan = __builtin_nanf("");
        for (int v = 0; v < MGPT_VOCAB; v++) dl[v] = nan;
        row_nll[r] = nan;
        return;
    }
    const float *l = logits + (int64_t)r * MGPT_VOCAB;
    float mx = l[0];
    for (int v = 1; v < MGPT_VOCAB; v++) mx = fmaxf(mx, l[v]);
    float sum = 0.f;
    for (int v = 0; v < MGPT_VOCAB; v++) sum += expf(l[v] - mx);
    const float lse = mx + logf(sum);
    for (int v = 0; v < MGPT_VOCAB; v++) {
        const float p = expf(l[v] - lse);
        dl[v] = (p - (v == tg ? 1.f : 0.f)) * k;
    }
    row_nll[r] = lse - l[tg];
}

__global__ void loss_final_rows_kernel(const double *__restrict__ acc, double n_rows, float *__restrict__ loss)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) loss[0] = (float)(acc[0] / n_rows);
}

// ----- attention of query 255 only (model.py:58-60), one workgroup per (row, head), thread j = key j -----
// TQ = float: the exact-fp32 path (s = (q . k) * scale, p = exp(s - m), statistics (m, 1 / l) as attn_bwd_q_kernel keeps them);
// TQ = uint16_t: the bf16 regime with the roundings attn_fwd_bf16_kernel / attn_bwd_bf16_kernel apply at query 255 -- q, k, v, y, dy are
// bf16, the statistics (max of q . k, 1 / sum of exp((q . k - max) * scale)) and every accumulator fp32; the forward's PV product takes
// bf16(exp(..)) and y = bf16(O / sum); the backward's dV takes bf16(P), dK and dq take bf16(dS), P = exp(..) / sum.
// q, y, dy, dq: compact [rows][C]; k, v: the head-major planes [rows][n_head][256][HS] of the general path; dk | dv: dense [tokens][3 C]
// columns [C, 3 C); stats [rows * n_head][2].  Matrix-vector work bound by one read of K and V.  Sums over the keys: each wave its 64
// keys by a fixed butterfly, the four waves in order; sums over keys per output d: 256 / HS groups of keys in order, the groups in order.
__device__ __forceinline__ float lastk_val(const float *p, int i) { return p[i]; }
__device__ __forceinline__ float lastk_val(const uint16_t *p, int i) { return __builtin_bit_cast(float, (unsigned)p[i] << 16); }
__device__ __forceinline__ float lastk_round(float v, const float *) { return v; }
__device__ __forceinline__ float lastk_round(float v, const uint16_t *) { return (float)(__bf16)v; }      // (nearest-even)
__device__ __forceinline__ void lastk_store(float *p, float v) { *p = v; }
__device__ __forceinline__ void lastk_store(uint16_t *p, float v) { *p = __builtin_bit_cast(uint16_t, (__bf16)v); }

// the key's row of HS elements into registers as fp32
template <int HS>
__device__ __forceinline__ void lastk_row(const float *p, float out[HS])
{
#pragma unroll
    for (int d = 0; d < HS; d += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p + d);
        out[d] = v.x; out[d + 1] = v.y; out[d + 2] = v.z; out[d + 3] = v.w;
    }
}
template <int HS>
__device__ __forceinline__ void lastk_row(const uint16_t *p, float out[HS])
{
#pragma unroll
    for (int d = 0; d < HS; d += 8) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p + d);
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            out[d + 2 * e] = __builtin_bit_cast(float, u[e] << 16);
            out[d + 2 * e + 1] = __builtin_bit_cast(float, u[e] & 0xffff0000u);
        }
    }
}

// s = q . k over d in order: the forward and the backward walk the same fmaf chain, so P is bit-identical in both
template <int HS>
__device__ __forceinline__ float lastk_dot(const float *__restrict__ a_lds, const float b[HS])
{
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HS; d++) s = fmaf(a_lds[d], b[d], s);
    return s;
}

// the sum of v over the workgroup's 256 threads in a fixed order; red: 4 floats of LDS; every thread gets the sum
__device__ __forceinline__ float lastk_sum256(float v, float *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                            // (red is free again)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float lastk_max256(float v, float *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// out[d] = sum_j w[j] * X[j][d] (w in LDS, X the (row, head)'s plane in memory, coalesced over d): thread (g, d) sums the keys of group g in
// order into part[g][d]; after a barrier the caller adds the groups in order
template <int HS, typename TQ>
__device__ __forceinline__ void lastk_weighted_rows(const float *w, const TQ *__restrict__ X, float *part)
{
    constexpr int NG = kT / HS, KPG = kT / NG;
    const int d = threadIdx.x % HS, g = threadIdx.x / HS;
    float acc = 0.f;
#pragma unroll 8
    for (int j = g * KPG; j < (g + 1) * KPG; j++) acc = fmaf(w[j], lastk_val(X, j * HS + d), acc);
    part[g * HS + d] = acc;
}

// DROP (dropout on P, site 1; mgpt_gpt_forward_backward_rows_drop): the masks of the general call at query 255 -- element
// ((row0 + row) * n_head + head) * 65536 + 255 * 256 + key, thread j = key j, one hash per four consecutive keys (the four threads of a
// quad compute the same one).  As attn_fwd_drop_kernel / attn_fwd_bf16_kernel<HS, true>: l sums over all keys, the mask zeroes exp(..)
// after it joined the sum (bf16: the masked value is rounded for the PV product), and y = s / l * sum_j m_j p_j v_j with s / l in fp32.
// Backward: dp_j = m_j s (dy . v_j), D = dy . y (it holds for the dropped y), ds_j = p_j (dp_j - D), dV_j = m_j s p_j dy (bf16: mask and
// scale in fp32 before P is rounded as the dV operand).
template <bool DROP>
__device__ __forceinline__ uint64_t lastk_hash(const Drop &dr, int bh, int j)
{
    if constexpr (DROP) return drop_hash_at(drop_base(dr.key, (dr.base >> 2) + (uint64_t)bh * (kT * kT / 4)), (uint32_t)((kT - 1) * kT + j) >> 2);
    else return 0;
}

template <int HS, typename TQ, bool DROP = false>
__global__ __launch_bounds__(256) void attn_last_fwd_kernel(const TQ *__restrict__ q, const TQ *__restrict__ kplane, const TQ *__restrict__ vplane,
                                                            TQ *__restrict__ y, float *__restrict__ stats, int n_head, float scale, Drop dr)
{
    constexpr bool BF = sizeof(TQ) == 2;
    constexpr int NG = kT / HS;
    __shared__ __attribute__((aligned(16))) float sq[HS], sp[kT], part[kT], red[4];
    const int bh = blockIdx.x, b = bh / n_head, head = bh - b * n_head, C = n_head * HS, j = threadIdx.x;
    const TQ *K = kplane + (int64_t)bh * kT * HS, *V = vplane + (int64_t)bh * kT * HS;
    if (j < HS) sq[j] = lastk_val(q, (int64_t)b * C + head * HS + j);
    float kr[HS];
    lastk_row<HS>(K + j * HS, kr);
    __syncthreads();
    float s = lastk_dot<HS>(sq, kr);
    if (!BF) s *= scale;
    const float m = lastk_max256(s, red);
    const float p = BF ? expf((s - m) * scale) : expf(s - m);
    const float l = lastk_sum256(p, red);
    if constexpr (DROP) sp[j] = drop_keep(lastk_hash<DROP>(dr, bh, j), j & 3, dr.thr) ? lastk_round(p, q) : 0.f;
    else sp[j] = lastk_round(p, q);
    __syncthreads();
    lastk_weighted_rows<HS, TQ>(sp, V, part);
    __syncthreads();
    const float inv_l = 1.f / l;
    if (j < HS) {
        float o = 0.f;
#pragma unroll
        for (int g = 0; g < NG; g++) o += part[g * HS + j];
        if constexpr (DROP) lastk_store(y + (int64_t)b * C + head * HS + j, o * (dr.scale / l));
        else lastk_store(y + (int64_t)b * C + head * HS + j, o * inv_l);
    }
    if (j == 0) { stats[(int64_t)bh * 2] = m; stats[(int64_t)bh * 2 + 1] = inv_l; }
}

template <int HS, typename TQ, bool DROP = false>
__global__ __launch_bounds__(256) void attn_last_bwd_kernel(const TQ *__restrict__ q, const TQ *__restrict__ kplane, const TQ *__restrict__ vplane,
                                                            const TQ *__restrict__ y, const TQ *__restrict__ dy, const float *__restrict__ stats,
                                                            float *__restrict__ dqkv, float *__restrict__ dq, int n_head, float scale, Drop dr)
{
    constexpr bool BF = sizeof(TQ) == 2;
    constexpr int NG = kT / HS;
    __shared__ __attribute__((aligned(16))) float sq[HS], sdy[HS], sy[HS], sds[kT], part[kT];
    const int bh = blockIdx.x, b = bh / n_head, head = bh - b * n_head, C = n_head * HS, j = threadIdx.x;
    const TQ *K = kplane + (int64_t)bh * kT * HS, *V = vplane + (int64_t)bh * kT * HS;
    if (j < HS) {
        const int64_t o = (int64_t)b * C + head * HS + j;
        sq[j] = lastk_val(q, o); sdy[j] = lastk_val(dy, o); sy[j] = lastk_val(y, o);
    }
    float kr[HS], vr[HS];
    lastk_row<HS>(K + j * HS, kr);
    lastk_row<HS>(V + j * HS, vr);
    const float m = stats[(int64_t)bh * 2], inv_l = stats[(int64_t)bh * 2 + 1];
    __syncthreads();
    float D = 0.f;                                              // rowsum(dy o y), every thread the same chain
#pragma unroll
    for (int d = 0; d < HS; d++) D = fmaf(sdy[d], sy[d], D);
    const float s = lastk_dot<HS>(sq, kr);
    const float p = (BF ? expf((s - m) * scale) : expf(s * scale - m)) * inv_l;
    float ds, pw;                                               // pw, dsw: the operands of dV, and of dK and dq
    if constexpr (DROP) {
        const float f = drop_factor(lastk_hash<DROP>(dr, bh, j), j & 3, dr);        // m s of (query 255, key j)
        ds = p * (lastk_dot<HS>(sdy, vr) * f - D);
        pw = lastk_round(p * f, q);
    } else {
        ds = p * (lastk_dot<HS>(sdy, vr) - D);
        pw = lastk_round(p, q);
    }
    const float dsw = lastk_round(ds, q);
    sds[j] = dsw;
    float *o = dqkv + ((int64_t)b * kT + j) * 3 * C + C + head * HS;       // dK_j, and dV_j at + C
#pragma unroll
    for (int d = 0; d < HS; d += 4) {
        *reinterpret_cast<float4 *>(o + d) =
            make_float4(dsw * sq[d] * scale, dsw * sq[d + 1] * scale, dsw * sq[d + 2] * scale, dsw * sq[d + 3] * scale);
        *reinterpret_cast<float4 *>(o + C + d) = make_float4(pw * sdy[d], pw * sdy[d + 1], pw * sdy[d + 2], pw * sdy[d + 3]);
    }
    __syncthreads();
    lastk_weighted_rows<HS, TQ>(sds, K, part);
    __syncthreads();
    if (j < HS) {
        float a = 0.f;
#pragma unroll
        for (int g = 0; g < NG; g++) a += part[g * HS + j];
        dq[(int64_t)b * C + head * HS + j] = a * scale;
    }
}

// ----- embedding backward (model.py:171-175) -----
// d wpe[t][c] += sum over rows of dx0[row][t][c], rows in order
__global__ __launch_bounds__(256) void wpe_bwd_kernel(const float *__restrict__ dx, int rows, int C, float *__restrict__ gwpe)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)kT * C) return;
    float s = 0.f;
    for (int r = 0; r < rows; r++) s += dx[(int64_t)r * kT * C + i];
    gwpe[i] += s;
}

// part[s][id][c] = sum over the tokens of slab s with token id `id` (blockIdx.x) of dx0[m][c], m in order, in double; no sort needed (67 ids)
__global__ __launch_bounds__(256) void wte_bwd_part_kernel(const uint8_t *__restrict__ tokens, const float *__restrict__ dx, int64_t M, int C,
                                                           int kps, float *__restrict__ part)
{
    const int id = blockIdx.x;
    const int64_t mb = (int64_t)blockIdx.y * kps, me = min<int64_t>(M, mb + kps);
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int64_t m = mb; m < me; m++)
            if (tokens[m] == id) s += (double)dx[m * C + c];
        part[((int64_t)blockIdx.y * MGPT_VOCAB + id) * C + c] = (float)s;
    }
}

// ----- gradient norm and AdamW over the parameter tensors; a block table splits every tensor into chunks of kChunk elements -----
constexpr int kChunk = 16384;
struct Blk {
    int64_t begin, end;     // element range in params / grads
    int tensor, decay;      // tensor index (its step counter), 1 = weight decay applies (configure_optimizers, model.py:209-214)
};

// part[b] = sum of g^2 over block b's range (double, fixed order)
__global__ __launch_bounds__(256) void sumsq_part_kernel(const float *__restrict__ g, const Blk *__restrict__ blk, double *__restrict__ part)
{
    __shared__ double sd[256];
    const Blk bk = blk[blockIdx.x];
    double s = 0.0;
    for (int64_t i = bk.begin + threadIdx.x; i < bk.end; i += 256) { const double v = g[i]; s += v * v; }
    sd[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sd[threadIdx.x] += sd[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sd[0];
}

// torch.nn.utils.clip_grad_norm_: total = || (||g_p||)_p ||, coef = min(max_norm / (total + 1e-6), 1); one thread, tensors and blocks in order
__global__ void clip_coef_kernel(const double *__restrict__ part, const Blk *__restrict__ blk, int n_blk, float max_norm,
                                 float *__restrict__ total_out, float *__restrict__ coef)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double tot = 0.0, cur = 0.0;
    for (int b = 0; b < n_blk; b++) {
        cur += part[b];
        if (b + 1 == n_blk || blk[b + 1].tensor != blk[b].tensor) {
            const double n = sqrt(cur);
            tot += n * n;
            cur = 0.0;
        }
    }
    const float total = (float)sqrt(tot);
    if (total_out) total_out[0] = total;
    coef[0] = fminf(max_norm / (total + 1e-6f), 1.0f);
}

__global__ __launch_bounds__(256) void scale_kernel(float *__restrict__ g, int64_t n, const float *__restrict__ coef)
{
    const float c = coef[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g[i] *= c;
}

__global__ void step_inc_kernel(float *__restrict__ steps, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) steps[i] += 1.f;
}

// torch.optim.AdamW (single-tensor, non-capturable): step += 1 (step_inc_kernel, before this);  p *= 1 - lr * wd;  m = lerp(m, g, 1 - b1);
// v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
__global__ __launch_bounds__(256) void adamw_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                                                    const Blk *__restrict__ blk, const float *__restrict__ steps, float lr, float b1, float b2,
                                                    float eps, float wd)
{
    const Blk bk = blk[blockIdx.x];
    const double t = (double)steps[bk.tensor];
    const float step_size = (float)((double)lr / (1.0 - pow((double)b1, t)));
    const float bc2s = (float)sqrt(1.0 - pow((double)b2, t));
    const float decay = bk.decay ? 1.0f - lr * wd : 1.0f;
    for (int64_t i = bk.begin + threadIdx.x; i < bk.end; i += 256) {
        const float gi = g[i];
        float pi = p[i] * decay;
        const float mi = fmaf(1.0f - b1, gi - m[i], m[i]);          // torch.lerp(m, g, 1 - b1) (weight < 0.5 form)
        const float vi = fmaf(v[i], b2, (1.0f - b2) * gi * gi);     // mul_(b2).addcmul_(g, g, value = 1 - b2)
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / bc2s + eps;
        pi = fmaf(-step_size, mi / denom, pi);
        p[i] = pi;
    }
}

}  // namespace trk
}  // namespace mgpt
