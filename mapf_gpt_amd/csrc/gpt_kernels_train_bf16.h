// gpt_kernels_train_bf16.h -- bf16 mixed-precision training kernels (mgpt_gpt_forward_backward_prec with MGPT_PREC_BF16, train.hip), gfx950.
//
// train.py:146-156 runs every micro-step under torch.amp.autocast(bfloat16): the five linears take bf16 operands and give bf16 outputs, GELU
// runs on bf16 tensors, LayerNorm, softmax statistics, cross-entropy and every accumulator stay fp32.  The kernels here are the matrix products
// of that regime on v_mfma_f32_16x16x32_bf16 (fp32 accumulate) -- the four block linears and attention -- and the LayerNorm backward with its
// gain sums.  GEMM operands are rounded to bf16 (round-to-nearest-even, = tensor.to(torch.bfloat16)) as they are loaded, so the fp32 master
// weights, the fp32 residual gradient and the saved fp32 LayerNorm outputs feed the MFMAs directly, and no bf16 weight copy exists to go stale.  No kernel uses a floating-point atomic and
// every sum runs in a fixed order: two identical calls give bit-identical gradients.
//
// GEMM: out(m, n) = sum_k A(m, k) * B(n, k).  A(m, k) = A[m * lda + k] (KC, k contiguous) or A[k * lda + m] (MC); B(n, k) likewise.  So
//   forward linear  out[m][n]  = X[m][k] W[n][k]          A = X KC,   B = W KC
//   input gradient  dX[m][k']  = dY[m][n] W[n][k']        A = dY KC,  B = W MC
//   weight gradient dW[n][k']  = sum_m dY[m][n] X[m][k']  A = dY MC,  B = X MC   (per token slab: grid z, fp32 partials [S][n][k'])
// A workgroup of 4 waves computes a 128 x 64 tile over k steps of 32: the operands are rounded and packed into LDS as [row][k] (MC operands are
// transposed in registers on the way), each wave computes 64 x 32 with 4 x 2 MFMAs per k step.  The MFMA takes the B fragment first, so a
// lane's four accumulators are four consecutive n of one m and every store is 8 or 16 bytes wide.
#pragma once
#include "common.h"
#include "gpt_kernels_train.h"      // trk::Drop: the dropout masks

namespace mgpt {
namespace tbk {

typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kT = 256;
constexpr int BM = 128, BN = 64, BK = 32, LDP = BK + 8;      // LDS row pitch in bf16 elements (80 bytes: 16-byte aligned rows)

// two floats -> one dword of two bf16 (round-to-nearest-even, the first value in the low half)
__device__ __forceinline__ unsigned pack2(float a, float b)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
}
__device__ __forceinline__ float bf_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }
__device__ __forceinline__ float bf_round(float v) { return bf_lo(pack2(v, 0.f)); }

__device__ __forceinline__ float gelu_f(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad(float a)
{
    return 0.5f * (1.0f + erff(a * 0.70710678118654752440f)) + a * expf(-0.5f * a * a) * 0.39894228040143267794f;
}

// 8 consecutive elements -> 4 packed dwords
__device__ __forceinline__ u32x4 load8(const float *p)
{
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
    return (u32x4){pack2(a.x, a.y), pack2(a.z, a.w), pack2(b.x, b.y), pack2(b.z, b.w)};
}
__device__ __forceinline__ u32x4 load8(const uint16_t *p) { return *reinterpret_cast<const u32x4 *>(p); }

// elements (k, k + 1) of 8 consecutive rows -> 8 dwords, row i's pair in d[i]
__device__ __forceinline__ void pairs8(const float *p0, const float *p1, unsigned d[8])
{
    const float4 a0 = reinterpret_cast<const float4 *>(p0)[0], a1 = reinterpret_cast<const float4 *>(p0)[1];
    const float4 b0 = reinterpret_cast<const float4 *>(p1)[0], b1 = reinterpret_cast<const float4 *>(p1)[1];
    d[0] = pack2(a0.x, b0.x); d[1] = pack2(a0.y, b0.y); d[2] = pack2(a0.z, b0.z); d[3] = pack2(a0.w, b0.w);
    d[4] = pack2(a1.x, b1.x); d[5] = pack2(a1.y, b1.y); d[6] = pack2(a1.z, b1.z); d[7] = pack2(a1.w, b1.w);
}
__device__ __forceinline__ void pairs8(const uint16_t *p0, const uint16_t *p1, unsigned d[8])
{
    const u32x4 a = *reinterpret_cast<const u32x4 *>(p0), b = *reinterpret_cast<const u32x4 *>(p1);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        d[2 * i] = (a[i] & 0xffffu) | (b[i] << 16);
        d[2 * i + 1] = (a[i] >> 16) | (b[i] & 0xffff0000u);
    }
}

// one operand tile of ROWS x BK into LDS [ROWS][LDP] (bf16), rows >= nrows zero
template <typename T, bool KC, int ROWS>
__device__ __forceinline__ void stage(const T *__restrict__ src, int64_t ld, int r0, int nrows, int k0, uint16_t *lds)
{
    if constexpr (KC) {
#pragma unroll
        for (int c = threadIdx.x; c < ROWS * BK / 8; c += 256) {
            const int row = c >> 2, kq = (c & 3) * 8, r = r0 + row;
            const u32x4 v = r < nrows ? load8(src + (int64_t)r * ld + k0 + kq) : (u32x4){0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4 *>(lds + row * LDP + kq) = v;
        }
    } else {
        // c -> (8-row group, k pair), row groups fastest: consecutive threads read consecutive 8-element runs of one source row
#pragma unroll
        for (int c = threadIdx.x; c < ROWS / 8 * (BK / 2); c += 256) {
            const int rg = c % (ROWS / 8), kp = c / (ROWS / 8), r = r0 + rg * 8;
            unsigned d[8];
            if (r < nrows) {
                pairs8(src + (int64_t)(k0 + 2 * kp) * ld + r, src + (int64_t)(k0 + 2 * kp + 1) * ld + r, d);
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) d[i] = 0u;
            }
#pragma unroll
            for (int i = 0; i < 8; i++) *reinterpret_cast<unsigned *>(lds + (rg * 8 + i) * LDP + 2 * kp) = d[i];
        }
    }
}

enum { E_F32 = 0, E_PART = 1, E_RESID = 2, E_FC = 3, E_GELU_BWD = 4, E_QKV = 5, E_B16 = 6, E_RESID_DROP = 7, E_RESID_DROP_LAST = 8 };

struct Epi {
    float *f32 = nullptr;           // E_F32 / E_PART / E_RESID output
    uint16_t *b16 = nullptr;        // E_FC: bf16(a); E_GELU_BWD: bf16 gradient of a; E_QKV: q | k | v planes; E_B16: bf16 output
    uint16_t *b16b = nullptr;       // E_FC: bf16(gelu(a))
    const float *res = nullptr;     // E_RESID: residual input
    const uint16_t *aux = nullptr;  // E_GELU_BWD: bf16(a)
    int64_t ldc = 0;                // row pitch of the outputs (elements)
    int C = 0, hs = 0, n_head = 0;  // E_QKV: head-major bf16 planes of plane elements each
    int64_t plane = 0;              // (E_RESID_DROP_LAST: the row pitch of the mask, 256 C, the output being the compact matrix)
    trk::Drop drop;                 // E_RESID_DROP: the branch's mask stream, base = the index of the chunk's first element
};

// four consecutive outputs (m, n .. n + 3)
template <int EPI>
__device__ __forceinline__ void epilogue(const Epi &ep, int64_t m, int n, f32x4 v, int M)
{
    const int64_t o = m * ep.ldc + n;
    if constexpr (EPI == E_F32) {
        *reinterpret_cast<float4 *>(ep.f32 + o) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (EPI == E_PART) {
        *reinterpret_cast<float4 *>(ep.f32 + (int64_t)blockIdx.z * M * ep.ldc + o) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (EPI == E_RESID) {
        // x + bf16(linear output): the sum is fp32, as x + y of a bf16 y under autocast
        const float4 r = *reinterpret_cast<const float4 *>(ep.res + o);
        *reinterpret_cast<float4 *>(ep.f32 + o) =
            make_float4(r.x + bf_round(v[0]), r.y + bf_round(v[1]), r.z + bf_round(v[2]), r.w + bf_round(v[3]));
    } else if constexpr (EPI == E_RESID_DROP) {
        // x + dropout(bf16(linear output)): bf16(m s bf16(o)), as nn.Dropout on a bf16 tensor; n is a multiple of 4: one hash
        const uint64_t h = trk::drop_hash(ep.drop.key, (ep.drop.base + (uint64_t)o) >> 2);
        const float4 r = *reinterpret_cast<const float4 *>(ep.res + o);
        *reinterpret_cast<float4 *>(ep.f32 + o) = make_float4(
            r.x + bf_round(bf_round(v[0]) * trk::drop_factor(h, 0, ep.drop)), r.y + bf_round(bf_round(v[1]) * trk::drop_factor(h, 1, ep.drop)),
            r.z + bf_round(bf_round(v[2]) * trk::drop_factor(h, 2, ep.drop)), r.w + bf_round(bf_round(v[3]) * trk::drop_factor(h, 3, ep.drop)));
    } else if constexpr (EPI == E_RESID_DROP_LAST) {
        // ... of the compact last layer: row m is token 255 of row m, whose mask elements lie ep.plane = 256 C apart; drop.base = the
        // element of compact row 0, column 0
        const uint64_t h = trk::drop_hash(ep.drop.key, (ep.drop.base + (uint64_t)m * (uint64_t)ep.plane + (uint64_t)n) >> 2);
        const float4 r = *reinterpret_cast<const float4 *>(ep.res + o);
        *reinterpret_cast<float4 *>(ep.f32 + o) = make_float4(
            r.x + bf_round(bf_round(v[0]) * trk::drop_factor(h, 0, ep.drop)), r.y + bf_round(bf_round(v[1]) * trk::drop_factor(h, 1, ep.drop)),
            r.z + bf_round(bf_round(v[2]) * trk::drop_factor(h, 2, ep.drop)), r.w + bf_round(bf_round(v[3]) * trk::drop_factor(h, 3, ep.drop)));
    } else if constexpr (EPI == E_FC) {
        const u32x2 a = {pack2(v[0], v[1]), pack2(v[2], v[3])};
        const u32x2 h = {pack2(gelu_f(bf_lo(a[0])), gelu_f(bf_hi(a[0]))), pack2(gelu_f(bf_lo(a[1])), gelu_f(bf_hi(a[1])))};
        *reinterpret_cast<u32x2 *>(ep.b16 + o) = a;
        *reinterpret_cast<u32x2 *>(ep.b16b + o) = h;
    } else if constexpr (EPI == E_GELU_BWD) {
        // d a = bf16(bf16(d h) * gelu'(a)), the fp32 arithmetic of the bf16 GELU backward
        const u32x2 a = *reinterpret_cast<const u32x2 *>(ep.aux + o);
        const u32x2 d = {pack2(bf_round(v[0]) * gelu_grad(bf_lo(a[0])), bf_round(v[1]) * gelu_grad(bf_hi(a[0]))),
                         pack2(bf_round(v[2]) * gelu_grad(bf_lo(a[1])), bf_round(v[3]) * gelu_grad(bf_hi(a[1])))};
        *reinterpret_cast<u32x2 *>(ep.b16 + o) = d;
    } else if constexpr (EPI == E_B16) {
        *reinterpret_cast<u32x2 *>(ep.b16 + o) = (u32x2){pack2(v[0], v[1]), pack2(v[2], v[3])};
    } else {
        // q | k | v into head-major bf16 planes [rows][n_head][256][hs] (attn_fwd_bf16_kernel, attn_bwd_bf16_kernel)
        const int which = n / ep.C, nn = n - which * ep.C, head = nn / ep.hs, d = nn - head * ep.hs;
        const int64_t b = m / kT, t = m - b * kT;
        uint16_t *dst = ep.b16 + which * ep.plane + ((b * ep.n_head + head) * kT + t) * ep.hs + d;
        *reinterpret_cast<u32x2 *>(dst) = (u32x2){pack2(v[0], v[1]), pack2(v[2], v[3])};
    }
}

// grid (cdiv(N, 64), cdiv(M, 128), slabs); k runs over [z * kps, min(K, (z + 1) * kps)), kps and K multiples of 32; M and N multiples of 16
template <typename TA, bool A_KC, typename TB, bool B_KC, int EPI>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(const TA *__restrict__ A, int64_t lda, const TB *__restrict__ B, int64_t ldb, int M,
                                                        int N, int K, int kps, Epi ep)
{
    __shared__ __attribute__((aligned(16))) uint16_t sA[BM * LDP];
    __shared__ __attribute__((aligned(16))) uint16_t sB[BN * LDP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave & 1, wn = wave >> 1;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
    const int kb = blockIdx.z * kps, ke = min(K, kb + kps);
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fk = 8 * (lane >> 4);
    for (int k0 = kb; k0 < ke; k0 += BK) {
        stage<TA, A_KC, BM>(A, lda, m0, M, k0, sA);
        stage<TB, B_KC, BN>(B, ldb, n0, N, k0, sB);
        __syncthreads();
        u32x4 af[4], bfr[2];
#pragma unroll
        for (int i = 0; i < 4; i++) af[i] = *reinterpret_cast<const u32x4 *>(sA + (wm * 64 + i * 16 + fr) * LDP + fk);
#pragma unroll
        for (int j = 0; j < 2; j++) bfr[j] = *reinterpret_cast<const u32x4 *>(sB + (wn * 32 + j * 16 + fr) * LDP + fk);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, bfr[j]), __builtin_bit_cast(b8, af[i]), acc[i][j], 0, 0, 0);
        __syncthreads();
    }
    // acc[i][j][r] = out(m = m0 + wm * 64 + i * 16 + (lane & 15), n = n0 + wn * 32 + j * 16 + 4 * (lane >> 4) + r)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int m = m0 + wm * 64 + i * 16 + fr;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int n = n0 + wn * 32 + j * 16 + 4 * (lane >> 4);
            if (n < N) epilogue<EPI>(ep, m, n, acc[i][j], M);
        }
    }
}

// ----- attention (model.py:58-60, non-causal, T = 256) on v_mfma_f32_16x16x32_bf16, one workgroup per (row, head) -----
// q, k, v: bf16 planes [rows][n_head][256][HS]; y and dy: bf16 [tokens][C]; stats: fp32 (max of q . k, 1 / sum of exp) per query.
// A 16 x 16 block of S^T = K Q^T leaves lane l with query l & 15 and keys 4 (l >> 4) + r (r < 4): for the product over keys that follows,
// the lane's keys of two adjacent key blocks ARE its eight k slots (slot i < 4: key 32 c + 4 g + i, slot 4 + i: key 32 c + 16 + 4 g + i,
// g = l >> 4), so P and dS feed the next MFMA from registers; the other operand is read from a transposed LDS image [d][token] at the same
// keys.  Every sum runs in a fixed order (no atomics).
constexpr int kTP = kT + 8;                                  // pitch of the transposed LDS images [d][token]

__device__ __forceinline__ void tr_store(uint16_t *img, int row, int d0, u32x4 v)    // 8 elements of token `row` into [d][token]
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        img[(d0 + 2 * i) * kTP + row] = (uint16_t)(v[i] & 0xffffu);
        img[(d0 + 2 * i + 1) * kTP + row] = (uint16_t)(v[i] >> 16);
    }
}
// A fragment of a transposed image: row d, the eight tokens of lane group g in the 32-token chunk c
__device__ __forceinline__ u32x4 tr_frag(const uint16_t *img, int d, int c, int g)
{
    const uint16_t *p = img + d * kTP + 32 * c + 4 * g;
    const u32x2 lo = *reinterpret_cast<const u32x2 *>(p), hi = *reinterpret_cast<const u32x2 *>(p + 16);
    return (u32x4){lo[0], lo[1], hi[0], hi[1]};
}
__device__ __forceinline__ u32x4 pack8(const float a[4], const float b[4])
{
    return (u32x4){pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(b[0], b[1]), pack2(b[2], b[3])};
}
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
}

template <int HS>
constexpr size_t attn_fwd_lds() { return (size_t)kT * (HS + 8) * 2 + (size_t)HS * kTP * 2; }
template <int HS>
constexpr size_t attn_bwd_lds() { return (size_t)3 * HS * kTP * 2 + (size_t)3 * kT * 4; }

// forward: wave w takes the queries [64 w, 64 w + 64) in blocks of 16: S^T (16 key blocks in registers), fp32 max and sum of exp, then
// O^T = V^T P^T over 8 chunks of 32 keys with bf16(P); y = bf16(O / sum)
// DROP (dropout on P, site 1): the mask is applied to the fp32 exp(s - max) after it joined the sum (the softmax sum runs over all keys), the
// masked value is rounded to bf16 as the PV operand, and the factor s joins 1 / sum in fp32
template <int HS, bool DROP = false>
__global__ __launch_bounds__(256) void attn_fwd_bf16_kernel(const uint16_t *__restrict__ qkv, int64_t plane, uint16_t *__restrict__ y,
                                                            float *__restrict__ stats, int n_head, float scale, trk::Drop dr)
{
    constexpr int KP = HS + 8, NJ = HS / 32, ND = HS / 16;
    extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
    uint16_t *sK = lds16, *sVt = lds16 + kT * KP;
    const int bh = blockIdx.x, b = bh / n_head, head = bh - b * n_head, C = n_head * HS;
    const uint16_t *Q = qkv + (int64_t)bh * kT * HS, *K = Q + plane, *V = Q + 2 * plane;
    for (int c = threadIdx.x; c < kT * HS / 8; c += 256) {
        const int row = c / (HS / 8), d0 = (c % (HS / 8)) * 8;
        *reinterpret_cast<u32x4 *>(sK + row * KP + d0) = *reinterpret_cast<const u32x4 *>(K + row * HS + d0);
        tr_store(sVt, row, d0, *reinterpret_cast<const u32x4 *>(V + row * HS + d0));
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, g = lane >> 4;
#pragma unroll 1
    for (int qb = wave * 4; qb < wave * 4 + 4; qb++) {
        const int q = qb * 16 + fr;
        u32x4 qf[NJ];
#pragma unroll
        for (int j = 0; j < NJ; j++) qf[j] = *reinterpret_cast<const u32x4 *>(Q + q * HS + 32 * j + 8 * g);
        f32x4 s[16];                                          // s[kb][r] = q . k of key 16 kb + 4 g + r
#pragma unroll
        for (int kb = 0; kb < 16; kb++) {
            s[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NJ; j++)
                s[kb] = mfma16(*reinterpret_cast<const u32x4 *>(sK + (kb * 16 + fr) * KP + 32 * j + 8 * g), qf[j], s[kb]);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 16; kb++)
#pragma unroll
            for (int r = 0; r < 4; r++) mx = fmaxf(mx, s[kb][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 16; kb++)
#pragma unroll
            for (int r = 0; r < 4; r++) { s[kb][r] = expf((s[kb][r] - mx) * scale); sum += s[kb][r]; }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        if constexpr (DROP) {
            const uint64_t hb = trk::drop_base(dr.key, (dr.base >> 2) + (uint64_t)bh * (kT * kT / 4));
            const uint32_t e0 = (uint32_t)q * kT + 4 * g;   // the lane's keys 16 kb + 4 g + r: one hash per key block
#pragma unroll
            for (int kb = 0; kb < 16; kb++) {
                const uint64_t h = trk::drop_hash_at(hb, (e0 + 16 * kb) >> 2);
#pragma unroll
                for (int r = 0; r < 4; r++) s[kb][r] = trk::drop_keep(h, r, dr.thr) ? s[kb][r] : 0.f;
            }
        }
        f32x4 o[ND];
#pragma unroll
        for (int db = 0; db < ND; db++) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const float p0[4] = {s[2 * c][0], s[2 * c][1], s[2 * c][2], s[2 * c][3]};
            const float p1[4] = {s[2 * c + 1][0], s[2 * c + 1][1], s[2 * c + 1][2], s[2 * c + 1][3]};
            const u32x4 pf = pack8(p0, p1);
#pragma unroll
            for (int db = 0; db < ND; db++) o[db] = mfma16(tr_frag(sVt, db * 16 + fr, c, g), pf, o[db]);
        }
        const float inv = 1.f / sum;                         // o[db][r] = O[query q][d = 16 db + 4 g + r] * sum
        const float oy = DROP ? inv * dr.scale : inv;
        uint16_t *yr = y + ((int64_t)b * kT + q) * C + head * HS;
#pragma unroll
        for (int db = 0; db < ND; db++)
            *reinterpret_cast<u32x2 *>(yr + db * 16 + 4 * g) = (u32x2){pack2(o[db][0] * oy, o[db][1] * oy), pack2(o[db][2] * oy, o[db][3] * oy)};
        if (g == 0) {
            stats[((int64_t)bh * kT + q) * 2] = mx;
            stats[((int64_t)bh * kT + q) * 2 + 1] = inv;
        }
    }
}

// backward: P = exp((q . k - max) * scale) / sum from the forward's statistics, D = rowsum(dy o y) in fp32, dS = P (dP - D).
// Phase 1, wave w owns the keys [32 w, 32 w + 32): S and dP = dy V^T per 16 x 16 block, dV^T += dy^T P and dK^T += Q^T dS over the
// queries in order.  Phase 2, wave w owns the queries [32 w, 32 w + 32): S^T and dP^T recomputed, dQ^T += K^T dS^T over the keys in order.
// dq | dk | dv (fp32) into dqkv [tokens][3 C]
// DROP: dV takes bf16(m s P), dP is masked and scaled in fp32 before dS = P (m s dP - D); D holds for the dropped y.  The mask of a 16 x 16
// block is generated where the block is used (per tile, nothing is kept per row)
template <int HS, bool DROP = false>
__global__ __launch_bounds__(512) void attn_bwd_bf16_kernel(const uint16_t *__restrict__ qkv, int64_t plane, const uint16_t *__restrict__ y,
                                                            const uint16_t *__restrict__ dy, const float *__restrict__ stats,
                                                            float *__restrict__ dqkv, int n_head, float scale, trk::Drop dr)
{
    constexpr int NJ = HS / 32, ND = HS / 16;
    extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
    uint16_t *sQt = lds16, *sDt = lds16 + HS * kTP, *sKt = lds16 + 2 * HS * kTP;
    float *sM = reinterpret_cast<float *>(lds16 + 3 * HS * kTP), *sIL = sM + kT, *sD = sIL + kT;
    const int bh = blockIdx.x, b = bh / n_head, head = bh - b * n_head, C = n_head * HS;
    const uint16_t *Q = qkv + (int64_t)bh * kT * HS, *K = Q + plane, *V = Q + 2 * plane;
    const int64_t tok0 = (int64_t)b * kT;
    const uint16_t *DO = dy + tok0 * C + head * HS, *O = y + tok0 * C + head * HS;
    for (int c = threadIdx.x; c < kT * HS / 8; c += 512) {
        const int row = c / (HS / 8), d0 = (c % (HS / 8)) * 8;
        tr_store(sQt, row, d0, *reinterpret_cast<const u32x4 *>(Q + row * HS + d0));
        tr_store(sKt, row, d0, *reinterpret_cast<const u32x4 *>(K + row * HS + d0));
        tr_store(sDt, row, d0, *reinterpret_cast<const u32x4 *>(DO + (int64_t)row * C + d0));
    }
    if (threadIdx.x < kT) {
        const int i = threadIdx.x;
        float D = 0.f;
#pragma unroll
        for (int d = 0; d < HS; d += 8) {
            const u32x4 a = *reinterpret_cast<const u32x4 *>(DO + (int64_t)i * C + d), o = *reinterpret_cast<const u32x4 *>(O + (int64_t)i * C + d);
#pragma unroll
            for (int e = 0; e < 4; e++) { D = fmaf(bf_lo(a[e]), bf_lo(o[e]), D); D = fmaf(bf_hi(a[e]), bf_hi(o[e]), D); }
        }
        sD[i] = D;
        sM[i] = stats[((int64_t)bh * kT + i) * 2];
        sIL[i] = stats[((int64_t)bh * kT + i) * 2 + 1];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, g = lane >> 4;
    float *out = dqkv + tok0 * 3 * C + head * HS;
    [[maybe_unused]] uint64_t hb = 0;                         // (DROP) the base of this (row, head)'s 65536 elements
    if constexpr (DROP) hb = trk::drop_base(dr.key, (dr.base >> 2) + (uint64_t)bh * (kT * kT / 4));
    {   // phase 1: dV, dK of the keys [32 wave, 32 wave + 32)
        u32x4 kf[2][NJ], vf[2][NJ];
#pragma unroll
        for (int kl = 0; kl < 2; kl++)
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const int key = (2 * wave + kl) * 16 + fr;
                kf[kl][j] = *reinterpret_cast<const u32x4 *>(K + key * HS + 32 * j + 8 * g);
                vf[kl][j] = *reinterpret_cast<const u32x4 *>(V + key * HS + 32 * j + 8 * g);
            }
        f32x4 dv[2][ND], dk[2][ND];
#pragma unroll
        for (int kl = 0; kl < 2; kl++)
#pragma unroll
            for (int db = 0; db < ND; db++) { dv[kl][db] = (f32x4){0.f, 0.f, 0.f, 0.f}; dk[kl][db] = dv[kl][db]; }
        for (int c = 0; c < 8; c++) {
            float p[2][2][4], ds[2][2][4];                    // [query block of the chunk][key block][r]
#pragma unroll
            for (int ql = 0; ql < 2; ql++) {
                const int qrow = (2 * c + ql) * 16 + fr;
                u32x4 qa[NJ], da[NJ];
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    qa[j] = *reinterpret_cast<const u32x4 *>(Q + qrow * HS + 32 * j + 8 * g);
                    da[j] = *reinterpret_cast<const u32x4 *>(DO + (int64_t)qrow * C + 32 * j + 8 * g);
                }
#pragma unroll
                for (int kl = 0; kl < 2; kl++) {
                    f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = sv;     // [query (2 c + ql) * 16 + 4 g + r][key (2 wave + kl) * 16 + fr]
#pragma unroll
                    for (int j = 0; j < NJ; j++) { sv = mfma16(qa[j], kf[kl][j], sv); dp = mfma16(da[j], vf[kl][j], dp); }
                    // (DROP) the block's 16 x 16 mask takes 64 hashes, one per lane: lane L hashes query (2 c + ql) * 16 + (L >> 2), keys
                    // (2 wave + kl) * 16 + 4 (L & 3) .. + 3 and keeps their four keep bits; a lane fetches the bits of its four queries
                    [[maybe_unused]] unsigned kbits = 0;
                    if constexpr (DROP) {
                        const uint64_t h = trk::drop_hash_at(hb, (uint32_t)(((2 * c + ql) * 16 + (lane >> 2)) * kT + (2 * wave + kl) * 16 + 4 * (lane & 3)) >> 2);
#pragma unroll
                        for (int i = 0; i < 4; i++) kbits |= (unsigned)trk::drop_keep(h, i, dr.thr) << i;
                    }
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int qi = (2 * c + ql) * 16 + 4 * g + r;
                        const float pr = expf((sv[r] - sM[qi]) * scale) * sIL[qi];
                        if constexpr (DROP) {
                            const float f = ((unsigned)__shfl((int)kbits, ((4 * g + r) << 2) | (fr >> 2)) >> (fr & 3)) & 1u ? dr.scale : 0.f;
                            p[ql][kl][r] = pr * f;
                            ds[ql][kl][r] = pr * (dp[r] * f - sD[qi]);
                        } else {
                            p[ql][kl][r] = pr;
                            ds[ql][kl][r] = pr * (dp[r] - sD[qi]);
                        }
                    }
                }
            }
#pragma unroll
            for (int kl = 0; kl < 2; kl++) {
                const u32x4 pf = pack8(p[0][kl], p[1][kl]), sf = pack8(ds[0][kl], ds[1][kl]);
#pragma unroll
                for (int db = 0; db < ND; db++) {
                    dv[kl][db] = mfma16(tr_frag(sDt, db * 16 + fr, c, g), pf, dv[kl][db]);
                    dk[kl][db] = mfma16(tr_frag(sQt, db * 16 + fr, c, g), sf, dk[kl][db]);
                }
            }
        }
#pragma unroll
        for (int kl = 0; kl < 2; kl++) {                      // dv[kl][db][r] = dV[key (2 wave + kl) * 16 + fr][d = 16 db + 4 g + r]
            float *o = out + (int64_t)((2 * wave + kl) * 16 + fr) * 3 * C;
#pragma unroll
            for (int db = 0; db < ND; db++) {
                const f32x4 v = dv[kl][db], k = dk[kl][db];
                *reinterpret_cast<float4 *>(o + 2 * C + db * 16 + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4 *>(o + C + db * 16 + 4 * g) = make_float4(k[0] * scale, k[1] * scale, k[2] * scale, k[3] * scale);
            }
        }
    }
    {   // phase 2: dQ of the queries [32 wave, 32 wave + 32)
        u32x4 qf[2][NJ], df[2][NJ];
        float mq[2], ilq[2], dq_[2];
#pragma unroll
        for (int ql = 0; ql < 2; ql++) {
            const int q = (2 * wave + ql) * 16 + fr;
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                qf[ql][j] = *reinterpret_cast<const u32x4 *>(Q + q * HS + 32 * j + 8 * g);
                df[ql][j] = *reinterpret_cast<const u32x4 *>(DO + (int64_t)q * C + 32 * j + 8 * g);
            }
            mq[ql] = sM[q]; ilq[ql] = sIL[q]; dq_[ql] = sD[q];
        }
        f32x4 dq[2][ND];
#pragma unroll
        for (int ql = 0; ql < 2; ql++)
#pragma unroll
            for (int db = 0; db < ND; db++) dq[ql][db] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < 8; c++) {
            float ds[2][2][4];                                // [query block][key block of the chunk][r]
#pragma unroll
            for (int kl = 0; kl < 2; kl++) {
                const int krow = (2 * c + kl) * 16 + fr;
                u32x4 ka[NJ], va[NJ];
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    ka[j] = *reinterpret_cast<const u32x4 *>(K + krow * HS + 32 * j + 8 * g);
                    va[j] = *reinterpret_cast<const u32x4 *>(V + krow * HS + 32 * j + 8 * g);
                }
#pragma unroll
                for (int ql = 0; ql < 2; ql++) {
                    f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpt = st;    // [key (2 c + kl) * 16 + 4 g + r][query (2 wave + ql) * 16 + fr]
                    uint64_t hq = 0;                              // (DROP) the four keys' hash
#pragma unroll
                    for (int j = 0; j < NJ; j++) { st = mfma16(ka[j], qf[ql][j], st); dpt = mfma16(va[j], df[ql][j], dpt); }
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if constexpr (DROP) {
                            if (r == 0) hq = trk::drop_hash_at(hb, (uint32_t)(((2 * wave + ql) * 16 + fr) * kT + (2 * c + kl) * 16 + 4 * g) >> 2);
                            ds[ql][kl][r] = expf((st[r] - mq[ql]) * scale) * ilq[ql] * (dpt[r] * trk::drop_factor(hq, r, dr) - dq_[ql]);
                        } else {
                            ds[ql][kl][r] = expf((st[r] - mq[ql]) * scale) * ilq[ql] * (dpt[r] - dq_[ql]);
                        }
                    }
                }
            }
#pragma unroll
            for (int ql = 0; ql < 2; ql++) {
                const u32x4 sf = pack8(ds[ql][0], ds[ql][1]);
#pragma unroll
                for (int db = 0; db < ND; db++) dq[ql][db] = mfma16(tr_frag(sKt, db * 16 + fr, c, g), sf, dq[ql][db]);
            }
        }
#pragma unroll
        for (int ql = 0; ql < 2; ql++) {
            float *o = out + (int64_t)((2 * wave + ql) * 16 + fr) * 3 * C;
#pragma unroll
            for (int db = 0; db < ND; db++) {
                const f32x4 v = dq[ql][db];
                *reinterpret_cast<float4 *>(o + db * 16 + 4 * g) = make_float4(v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale);
            }
        }
    }
}

// ----- LayerNorm backward (eps 1e-5, gain only) with the gain's column sums: one wavefront per token, kLnTok tokens per workgroup -----
// dres[m] (+)= rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dxn * w;  part[blockIdx.x][c] = sum over the workgroup's tokens of
// dxn * xhat (each wave its tokens in order, then the four waves in order).  colsum_reduce_kernel adds the partials in order.
constexpr int kLnTokPerWave = 32, kLnTok = 4 * kLnTokPerWave, kLnMaxJ = 12;     // C <= 64 * 12 = 768

template <bool ADD>
__global__ __launch_bounds__(256) void ln_bwd_gain_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ dxn,
                                                          float *__restrict__ dres, float *__restrict__ part, int64_t n_tok, int C)
{
    __shared__ float sg[4][64 * kLnMaxJ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float gacc[kLnMaxJ];
#pragma unroll
    for (int j = 0; j < kLnMaxJ; j++) gacc[j] = 0.f;
    const int64_t t0 = (int64_t)blockIdx.x * kLnTok + wave * kLnTokPerWave;
    for (int it = 0; it < kLnTokPerWave; it++) {
        const int64_t tok = t0 + it;
        if (tok >= n_tok) break;
        const float *px = x + tok * C, *pd = dxn + tok * C;
        float xv[kLnMaxJ], dv[kLnMaxJ];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < kLnMaxJ; j++) {
            const int c = lane + 64 * j;
            xv[j] = c < C ? px[c] : 0.f;
            dv[j] = c < C ? pd[c] * w[c] : 0.f;
            s += xv[j];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s / (float)C;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < kLnMaxJ; j++) {
            const float d = lane + 64 * j < C ? xv[j] - mean : 0.f;
            q = fmaf(d, d, q);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
        const float rstd = rsqrtf(q / (float)C + 1e-5f);
        float sg_ = 0.f, sgx = 0.f;
#pragma unroll
        for (int j = 0; j < kLnMaxJ; j++) {
            xv[j] = (xv[j] - mean) * rstd;                 // xhat (unused past C)
            sg_ += dv[j];
            sgx = fmaf(dv[j], xv[j], sgx);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { sg_ += __shfl_xor(sg_, o); sgx += __shfl_xor(sgx, o); }
        const float mg = sg_ / (float)C, mgx = sgx / (float)C;
#pragma unroll
        for (int j = 0; j < kLnMaxJ; j++) {
            const int c = lane + 64 * j;
            if (c < C) {
                const float dx = rstd * (dv[j] - mg - xv[j] * mgx);
                if (ADD) dres[tok * C + c] += dx; else dres[tok * C + c] = dx;
                gacc[j] = fmaf(pd[c], xv[j], gacc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kLnMaxJ; j++)
        if (lane + 64 * j < C) sg[wave][lane + 64 * j] = gacc[j];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256)
        part[(int64_t)blockIdx.x * C + c] = (sg[0][c] + sg[1][c]) + (sg[2][c] + sg[3][c]);
}

// out[c] += sum_{p < P} part[p][c]: 16 lanes per column take every 16th partial in order, then their 16 sums are added in order
__global__ __launch_bounds__(1024) void colsum_reduce_kernel(const float *__restrict__ part, int P, int C, float *__restrict__ out)
{
    __shared__ float s[16][64];
    const int cl = threadIdx.x & 63, r = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    float acc = 0.f;
    if (c < C)
        for (int p = r; p < P; p += 16) acc += part[(int64_t)p * C + c];
    s[r][cl] = acc;
    __syncthreads();
    if (r == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; i++) t += s[i][cl];
        out[c] += t;
    }
}

}  // namespace tbk
}  // namespace mgpt
