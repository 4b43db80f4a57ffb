// gpt_kernels_seq.h -- the head of EVERY position (GPT.forward(idx, targets), model.py:178-184) and the scoring of the last one.
//
// head_seq_kernel: ln_f (fp32, eps 1e-5, ln_f.bias of bias = True checkpoints) + tied lm_head (wte^T, 67 columns padded to 80) on every
// token of a row, optional logits [rows][T][67], and per row the sum of -log softmax(logits)[target] over the targeted positions and their
// count.  One workgroup per row (grid-stride over rows), eight waves of 32 positions; no float atomics: the row sums are a fixed
// shuffle tree and a fixed-order sum of the eight waves, whatever the grid.
//
// The product runs on v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fmaf chain).  Lane l = (i = l & 15, kq = l >> 4) owns token i of
// a 16-token tile and the column quarter kq: at k-step s it feeds column kq * C/4 + s as k-slot kq of both operands, so it streams its own
// token's row with 16-byte loads in either residual layout.  wte^T lives in LDS in slices of 4 x kSeqS columns ([kq][s][80], padded
// per quarter so the four quarters read different banks): one slice (loaded once per workgroup) for C <= 256, three for C = 768.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace mgpt {
namespace seqk {

constexpr int kV = 67;
constexpr int kVP = 80;                              // 5 column tiles of 16
constexpr int kSeqS = 64;                            // k-steps per lane quarter per LDS slice (4 x 64 = 256 columns)
constexpr int kSeqWaves = 8;                         // 8 waves x 32 positions = one 256-token row
__host__ __device__ constexpr int seq_kq_stride(int S) { return S * kVP + 16; }
// dynamic LDS of a launch for n_embd C: the wte^T slice + the per-wave row partial sums
__host__ __device__ constexpr size_t seq_lds_bytes(int C)
{
    return (size_t)4 * seq_kq_stride((C / 4) < kSeqS ? (C / 4) : kSeqS) * sizeof(float) + 2 * kSeqWaves * sizeof(float);
}

using f32x4s = __attribute__((ext_vector_type(4))) float;

// = fastk::xt_off (gpt_kernels_fast.h): chunk-major residual stream [M / 32][C / 8][32 tokens][8 floats]
__device__ __forceinline__ int64_t seq_xt_off(int64_t m, int n, int C) { return (((m >> 5) * (C >> 3) + (n >> 3)) << 8) + ((m & 31) << 3) + (n & 7); }

template <int TILED>
__device__ __forceinline__ f32x4s seq_ld4(const float *__restrict__ x, int64_t m, int col, int C)
{
    return *reinterpret_cast<const f32x4s *>(x + (TILED ? seq_xt_off(m, col, C) : m * C + col));
}

__device__ __forceinline__ float seq_sum16(float v)   // over the 16 lanes of one kq group
{
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ float seq_max16(float v)
{
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// x: residual after the last block, rows * T tokens (TILED: fastk::xt_off layout, T = 256).  logits / targets / row_nll / row_count may be
// NULL (targets == NULL <=> row_nll == NULL <=> row_count == NULL).  Targets outside [-1, kV): NaN in the row's sum (counted).
template <int TILED>
__global__ __launch_bounds__(512) void head_seq_kernel(const float *__restrict__ x, const float *__restrict__ lnf, const float *__restrict__ lnf_b,
                                                       const float *__restrict__ wte, int C, int rows, int T, float *__restrict__ logits,
                                                       const int32_t *__restrict__ targets, float *__restrict__ row_nll,
                                                       int32_t *__restrict__ row_count)
{
    extern __shared__ __attribute__((aligned(16))) float seq_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = lane & 15, kq = lane >> 4;
    const int Q = C >> 2;                                   // columns of one lane quarter
    const int S = Q < kSeqS ? Q : kSeqS;                    // k-steps per slice
    const int n_slices = (Q + S - 1) / S;
    const int kqs = seq_kq_stride(S);
    float *wl = seq_lds;                                    // [4][kqs]
    float *red = seq_lds + 4 * kqs;                         // [kSeqWaves] nll sums, [kSeqWaves] counts
    const int p0 = wave * 32;
    const bool active = p0 < T;                             // (wave-uniform)
    bool staged = false;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        // ---- LayerNorm statistics of the wave's 2 x 16 tokens: each lane sums its quarter, the 4 quarters meet by shuffles ----
        float mean[2] = {0.f, 0.f}, rstd[2] = {0.f, 0.f};
        int64_t m[2];
#pragma unroll
        for (int mt = 0; mt < 2; mt++) {
            const int pos = min(p0 + mt * 16 + i, T - 1);   // (positions beyond T compute on a valid row and are dropped)
            m[mt] = (int64_t)row * T + pos;
        }
        if (active) {
#pragma unroll
            for (int mt = 0; mt < 2; mt++) {
                float s = 0.f;
                for (int c = 0; c < Q; c += 4) {
                    const f32x4s v = seq_ld4<TILED>(x, m[mt], kq * Q + c, C);
                    s += (v[0] + v[1]) + (v[2] + v[3]);
                }
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                mean[mt] = s / (float)C;
                float q = 0.f;
                for (int c = 0; c < Q; c += 4) {
                    const f32x4s v = seq_ld4<TILED>(x, m[mt], kq * Q + c, C);
#pragma unroll
                    for (int j = 0; j < 4; j++) { const float d = v[j] - mean[mt]; q = fmaf(d, d, q); }
                }
                q += __shfl_xor(q, 16);
                q += __shfl_xor(q, 32);
                rstd[mt] = rsqrtf(q / (float)C + 1e-5f);
            }
        }
        f32x4s acc[2][5];
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int n = 0; n < 5; n++) acc[mt][n] = f32x4s{0.f, 0.f, 0.f, 0.f};
        for (int sl = 0; sl < n_slices; sl++) {
            const int s0 = sl * S, slen = min(S, Q - s0);
            if (n_slices > 1 || !staged) {                  // (block-uniform) wte^T slice -> LDS: wl[kq][ss][v] = wte[v][kq * Q + s0 + ss]
                __syncthreads();
                const int per_v = 4 * slen;
                for (int e = tid; e < kVP * per_v; e += 512) {
                    const int v = e / per_v, rem = e - v * per_v, q4 = rem / slen, ss = rem - q4 * slen;
                    wl[q4 * kqs + ss * kVP + v] = v < kV ? wte[(size_t)v * C + q4 * Q + s0 + ss] : 0.f;
                }
                __syncthreads();
                staged = true;
            }
            if (!active) continue;
            const float *wq = wl + kq * kqs + i;
            for (int c = 0; c < slen; c += 4) {
                const int col = kq * Q + s0 + c;
                const f32x4s g = *reinterpret_cast<const f32x4s *>(lnf + col);
                f32x4s bb = {0.f, 0.f, 0.f, 0.f};
                if (lnf_b != nullptr) bb = *reinterpret_cast<const f32x4s *>(lnf_b + col);
                f32x4s a[2];
#pragma unroll
                for (int mt = 0; mt < 2; mt++) {
                    const f32x4s v = seq_ld4<TILED>(x, m[mt], col, C);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        float o = (v[j] - mean[mt]) * rstd[mt] * g[j];
                        if (lnf_b != nullptr) o += bb[j];
                        a[mt][j] = o;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
#pragma unroll
                    for (int n = 0; n < 5; n++) {
                        const float b = wq[(c + j) * kVP + n * 16];
                        acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][j], b, acc[0][n], 0, 0, 0);
                        acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][j], b, acc[1][n], 0, 0, 0);
                    }
                }
            }
        }
        // ---- epilogue: acc[mt][n][r] = logit of position p0 + 16 mt + 4 kq + r at vocabulary column 16 n + i ----
        float wsum = 0.f, wcnt = 0.f;
        if (active) {
#pragma unroll
            for (int mt = 0; mt < 2; mt++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int pos = p0 + mt * 16 + kq * 4 + r;
                    const bool valid = pos < T;
                    const int64_t tok = (int64_t)row * T + pos;
                    if (logits != nullptr && valid) {
#pragma unroll
                        for (int n = 0; n < 5; n++)
                            if (n < 4 || i < kV - 64) logits[tok * kV + n * 16 + i] = acc[mt][n][r];
                    }
                    if (targets != nullptr) {
                        const int t = valid ? targets[tok] : -1;
                        float mx = -INFINITY;
#pragma unroll
                        for (int n = 0; n < 5; n++)
                            if (n < 4 || i < kV - 64) mx = fmaxf(mx, acc[mt][n][r]);
                        mx = seq_max16(mx);
                        float se = 0.f, tl = 0.f;
#pragma unroll
                        for (int n = 0; n < 5; n++)
                            if (n < 4 || i < kV - 64) {
                                se += expf(acc[mt][n][r] - mx);
                                if (n * 16 + i == t) tl = acc[mt][n][r];
                            }
                        se = seq_sum16(se);
                        tl = seq_sum16(tl);                 // (one lane holds the target column, the others add zeros)
                        if (t != -1) {
                            wsum += (t >= 0 && t < kV) ? (mx + logf(se)) - tl : NAN;
                            wcnt += 1.f;
                        }
                    }
                }
            }
            wsum += __shfl_xor(wsum, 16);
            wsum += __shfl_xor(wsum, 32);
            wcnt += __shfl_xor(wcnt, 16);
            wcnt += __shfl_xor(wcnt, 32);
        }
        if (targets != nullptr) {
            if (lane == 0) { red[wave] = wsum; red[kSeqWaves + wave] = wcnt; }
            __syncthreads();
            if (tid == 0) {
                float s = 0.f, c = 0.f;
                for (int w = 0; w < kSeqWaves; w++) { s += red[w]; c += red[kSeqWaves + w]; }
                row_nll[row] = s;
                row_count[row] = (int32_t)c;
            }
            __syncthreads();
        }
    }
}

// Scoring against one action per row: nll[r] = -log softmax(logits[r])[target[r]] over all kV logits, hit[r] = (greedy action == target[r])
// with the greedy action of sample_kernel (gpt.hip): the first maximum of logits[0 .. n_actions).  Targets outside [0, kV): NaN, no hit.
__global__ __launch_bounds__(256) void score_last_kernel(const float *__restrict__ logits, int rows, const int32_t *__restrict__ targets,
                                                         float *__restrict__ nll, int32_t *__restrict__ hit, int n_actions)
{
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const float *l = logits + (size_t)row * kV;
    float mx = -INFINITY;
    int best = 0;
    for (int a = 0; a < n_actions; a++) {
        const float v = l[a];
        if (v > mx) { mx = v; best = a; }            // first maximum, as sample_kernel's greedy branch
    }
    const int t = targets[row];
    if (t < 0 || t >= kV) { nll[row] = NAN; hit[row] = 0; return; }
    float lm = -INFINITY;
    for (int v = 0; v < kV; v++) lm = fmaxf(lm, l[v]);
    float se = 0.f;
    for (int v = 0; v < kV; v++) se += expf(l[v] - lm);
    nll[row] = (lm + logf(se)) - l[t];
    hit[row] = best == t ? 1 : 0;
}

}  // namespace seqk
}  // namespace mgpt
