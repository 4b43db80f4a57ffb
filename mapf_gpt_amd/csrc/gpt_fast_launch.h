// gpt_fast_launch.h -- host launchers of the 16-bit forward's GEMM, LayerNorm and embedding kernels (gpt_kernels_fast.h): each checks the
// shape, picks the template instance and the dynamic LDS size, and launches on the given stream.  Which of them a call runs, and in which
// order, is gpt_plan.h's and gpt_fast.hip's business (make_plan / forward_chunk).
#pragma once
#include <algorithm>

#include "common.h"
#include "gpt_kernels_fast.h"

namespace mgpt {

template <class T, int NP, int PRO, int EPI>
int launch_gemm16(fastk::GemmArgs a, int C, hipStream_t s)
{
    MGPT_REQUIRE(a.M % 128 == 0 && a.K % 32 == 0, MGPT_ERR_UNSUPPORTED, "gemm16 shape M=%d K=%d", a.M, a.K);
    const int mt = a.M / 128;
    if (C == 160 && a.N % 160 == 0) {
        a.n_tiles_n = a.N / 160;
        hipLaunchKernelGGL((fastk::gemm16_kernel<T, NP, 160, 4, 1, PRO, EPI>), dim3(mt * a.n_tiles_n), dim3(256), 0, s, a);
    } else if (C == 64 && a.N % 64 == 0) {
        a.n_tiles_n = a.N / 64;
        hipLaunchKernelGGL((fastk::gemm16_kernel<T, NP, 64, 4, 1, PRO, EPI>), dim3(mt * a.n_tiles_n), dim3(256), 0, s, a);
    } else if (a.N % 128 == 0) {
        a.n_tiles_n = a.N / 128;
        if (EPI == fastk::EPI_RESID) a.stats_out = nullptr;          // rows span two waves: stats come from row_stats_kernel
        hipLaunchKernelGGL((fastk::gemm16_kernel<T, NP, 128, 2, 2, PRO, EPI>), dim3(mt * a.n_tiles_n), dim3(256), 0, s, a);
    } else {
        set_error("gemm16: N=%d unsupported for C=%d", a.N, C);
        return MGPT_ERR_UNSUPPORTED;
    }
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// one instance of the packed GEMM: gemm_pk16_kernel (K16: 16 x 16 x 32 MFMA, one-plane mode) or gemm_pk_kernel, NWV waves of 64 x 128
template <class T, int NP, int EPI, bool K16, int NWV, bool LNF>
void launch_gemm_pk_instance(const fastk::GemmArgs &a, unsigned grid, size_t lds, hipStream_t s)
{
    if constexpr (K16) hipLaunchKernelGGL((fastk::gemm_pk16_kernel<T, EPI, NWV, LNF>), dim3(grid), dim3(NWV * 64), lds, s, a);
    else hipLaunchKernelGGL((fastk::gemm_pk_kernel<T, NP, EPI, NWV, 0, LNF>), dim3(grid), dim3(NWV * 64), lds, s, a, (unsigned long long *)nullptr);
}

// ... chosen by (folded LayerNorm, half tiles); extra = gemm_pk_lds_extra behind either ring
template <class T, int NP, int EPI, bool K16>
void launch_gemm_pk_tiles(const fastk::GemmArgs &a, bool lnf, bool half_tiles, unsigned grid8, unsigned grid4, size_t extra, hipStream_t s)
{
    const size_t lds8 = (size_t)fastk::gemm_pk_lds(NP) + extra, lds4 = (size_t)fastk::gemm_pk_lds(NP, 4, EPI) + extra;
    if (lnf && half_tiles) launch_gemm_pk_instance<T, NP, EPI, K16, 4, true>(a, grid4, lds4, s);
    else if (lnf) launch_gemm_pk_instance<T, NP, EPI, K16, 8, true>(a, grid8, lds8, s);
    else if (half_tiles) launch_gemm_pk_instance<T, NP, EPI, K16, 4, false>(a, grid4, lds4, s);
    else launch_gemm_pk_instance<T, NP, EPI, K16, 8, false>(a, grid8, lds8, s);
}

// n_cu: compute units of the model's device (grid of the persistent instances)
template <class T, int NP, int EPI>
int launch_gemm_pk(fastk::GemmArgs a, int n_cu, hipStream_t s, bool half_tiles = false, bool big_call = true)
{
    constexpr int NST = fastk::gemm_pk_nst(NP, 8, EPI), KPS = fastk::gemm_pk_kps(NP);
    MGPT_REQUIRE(a.M % 256 == 0 && a.N % 256 == 0 && a.K % 32 == 0 && a.K >= 16 * KPS * NST, MGPT_ERR_UNSUPPORTED,
                 "gemm_pk shape M=%d N=%d K=%d", a.M, a.N, a.K);
    a.n_tiles_n = a.N / 256;
    if (EPI == fastk::EPI_RESID) a.stats_out = nullptr;               // rows span two waves: stats come from row_stats_kernel
    const bool lut = EPI == fastk::EPI_GELU && a.gelu_lut != nullptr;
    const bool lnf = EPI != fastk::EPI_RESID && a.ln_stats != nullptr;
    const size_t extra = (size_t)fastk::gemm_pk_lds_extra(lnf, lut);  // (folded LayerNorm: the Phi table slot is always reserved)
    // half_tiles (small launches: one environment's rows are 32 tiles of 256 rows per column tile, which leaves most CUs idle): 128-row tiles, 4 waves,
    // two workgroups per CU -- same arithmetic per token (a wave's 64 x 128 sub-tile and its k order do not change)
    const int tiles8 = (a.M / 256) * a.n_tiles_n, tiles4 = (a.M / 128) * a.n_tiles_n;
    if constexpr (NP == 1) {
        // one-plane mode: the same GEMM on v_mfma_f32_16x16x32 (gpt_kernels_fast.h: gemm_pk16_kernel), one workgroup per tile
        // -- in LARGE calls only: a 32-row forward is not at the power limit, and there the 12 % more cycles per flop of the small shape show (2.49 -> 2.71 ms);
        // the choice is a property of the call (as for the other small-launch kernels), so every chunk of a call runs the same arithmetic
        if (big_call && a.K % 64 == 0 && a.K >= 128 && (EPI != fastk::EPI_GELU || lut)) {
            launch_gemm_pk_tiles<T, NP, EPI, true>(a, lnf, half_tiles, (unsigned)tiles8, (unsigned)tiles4, extra, s);
            MGPT_LAUNCH_CHECK();
            return MGPT_OK;
        }
    }
    MGPT_REQUIRE(!lnf || EPI != fastk::EPI_GELU || lut, MGPT_ERR_STATE, "%s", "folded LayerNorm: the GELU epilogue needs the Phi table");
    const bool persist = fastk::gemm_pk_persistent(NP, EPI, lnf);    // one workgroup per CU walking the tiles (gpt_kernels_fast.h: gemm_pk_kernel)
    launch_gemm_pk_tiles<T, NP, EPI, false>(a, lnf, half_tiles, (unsigned)(persist ? std::min(tiles8, n_cu) : tiles8),
                                            (unsigned)(persist ? std::min(tiles4, 2 * n_cu) : tiles4), extra, s);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// ---- one dispatch on C per kernel that is compiled for a fixed row width ----
// stats, mean != NULL: the raw mode of ln_pack_kernel (folded LayerNorm: once per forward, for the embedding rows)
template <class T, int NP>
int launch_ln_pack(const float *x, const float *gain, uint16_t *out, int64_t M, int C, int tiled, hipStream_t s, float2 *stats = nullptr,
                   float *mean = nullptr)
{
    ProfScope ps(P_LAYERNORM, s);
#define MGPT_LN_PACK(KSW_) hipLaunchKernelGGL((fastk::ln_pack_kernel<T, NP, KSW_>), dim3((unsigned)(M / 32)), dim3(256), 0, s, x, gain, out, C, tiled, stats, mean)
    if (C == 256) MGPT_LN_PACK(4); else if (C == 512) MGPT_LN_PACK(8); else if (C == 768) MGPT_LN_PACK(12); else if (C == 1024) MGPT_LN_PACK(16);
    else { set_error("ln_pack: C=%d unsupported", C); return MGPT_ERR_UNSUPPORTED; }
#undef MGPT_LN_PACK
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// KERNEL_<NV>: NV = float4s of a row per lane
#define MGPT_BY_ROW_WIDTH(KERNEL_, ...)                                                                                        \
    do {                                                                                                                       \
        if (C <= 256) hipLaunchKernelGGL((fastk::KERNEL_<1>), grid, dim3(256), 0, s, __VA_ARGS__);                              \
        else if (C <= 512) hipLaunchKernelGGL((fastk::KERNEL_<2>), grid, dim3(256), 0, s, __VA_ARGS__);                         \
        else if (C <= 768) hipLaunchKernelGGL((fastk::KERNEL_<3>), grid, dim3(256), 0, s, __VA_ARGS__);                         \
        else hipLaunchKernelGGL((fastk::KERNEL_<4>), grid, dim3(256), 0, s, __VA_ARGS__);                                       \
    } while (0)

inline int launch_row_stats(const float *x, float2 *stats, int64_t n_tok, int C, hipStream_t s)
{
    ProfScope ps(P_LAYERNORM, s);
    const dim3 grid((unsigned)cdiv64(n_tok, 4));
    MGPT_BY_ROW_WIDTH(row_stats_kernel, x, stats, n_tok, C);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

inline int launch_embed_stats(const uint8_t *tokens, const float *wte, const float *wpe, float *x, float2 *stats, int64_t n_tok, int C, hipStream_t s)
{
    ProfScope ps(P_EMBED, s);
    const dim3 grid((unsigned)cdiv64(n_tok, 4));
    MGPT_BY_ROW_WIDTH(embed_stats_kernel, tokens, wte, wpe, x, stats, n_tok, C);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}
#undef MGPT_BY_ROW_WIDTH

inline bool fused_stats(int C) { return C == 160 || C == 64; }

}  // namespace mgpt
