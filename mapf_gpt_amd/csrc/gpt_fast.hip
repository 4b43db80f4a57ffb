// gpt_fast.hip -- host side of the 16-bit-MFMA forward (MGPT_PREC_F16X3 / MGPT_PREC_BF16):
// weight plane packing at finalize, workspace, and the per-chunk launch sequence
//   embed+stats -> L x { LN1+QK gemm, LN1+V^T gemm, attention, proj+residual(+stats),
//                        LN2+FC+GELU gemm, proj2+residual(+stats) } -> ln_f + head (fp32 kernel)
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "gpt_ctx.h"                // (includes gpt_plan.h: Family, ModeFacts, Plan; mode_facts at build, make_plan per chunk)
#include "gpt_kernels_fast.h"
#include "gpt_fast_launch.h"        // launch_gemm16, launch_gemm_pk, launch_ln_pack, launch_row_stats, launch_embed_stats
#include "gpt_kernels_c256q.h"      // (includes gpt_kernels_c256p.h)
#include "gpt_kernels_fused16.h"
#include "gpt_kernels_c256b.h"      // attn256q_kernel (includes gpt_kernels_c256.h)
#include "gpt_kernels_c160p.h"
#include "gpt_kernels_c160a.h"
#include "gpt_kernels_last.h"

using namespace mgpt;

namespace {

constexpr int kT = 256;
constexpr int kV = MGPT_VOCAB;

struct PlaneSet {           // one weight matrix [N][K] as 16-bit planes
    uint16_t *hi = nullptr, *lo = nullptr;
    float inv_scale = 1.f;
};

struct ModeState {          // one precision mode: what dispatch depends on, and the buffers grouped by the ModeBuilder function that fills them
    bool built = false;
    ModeFacts facts = {};
    struct Planes {         // build_planes (every family): the four matrices of a layer as row-major planes, the Phi table of the fused MLP kernels (kGeluLutN pairs)
        std::vector<PlaneSet> attn, proj, fc, proj2;
        float2 *gelu_lut = nullptr;
    } pl;
    struct SixM {           // build_6m (FAM_6M)
        // mlp256p_kernel's cyclic weight stream in consumption order (LayerNorm gain folded into c_fc), per layer [period step][pair][plane][lane][8];
        // the same stream in the fragment layout of mlp256q_kernel (16 x 16 x 32 MFMA: large calls); 1 / the scale c_fc * gain was packed with
        std::vector<uint16_t *> mlp256_pk, mlp256q_pk;
        std::vector<float2 *> mlp256_lut;          // per layer: the Phi table times 1 / scale of the layer's c_fc stream (mlp256p_kernel)
        std::vector<uint16_t *> attn256_pk;        // attn256_kernel's c_attn stream in consumption order, per layer (small calls)
        std::vector<float> mlp256_inv1, attn256_inv;   // 1 / scale of the mlp256 streams and of the attn256 streams (c_attn.weight * ln_1.weight)
        // attn256q_kernel (whole attention block, persistent: gpt_kernels_c256b.h): c_attn + c_proj stream per layer, and the per-workgroup spill slab
        std::vector<uint16_t *> attn256q_pk;
        unsigned char *attn256q_spill = nullptr;
        // layer 0's q | k | v per (position, token) pair (attn256q_kernel<.., TAB = 2>), built from attn256q_pk[0]; facts.l0_qkv_table
        unsigned char *l0_table = nullptr;
    } m6;
    struct Register {       // build_register (C = 64 / 160)
        // the fused MLP's packed stream per layer, [hidden tile][fragment][plane][lane][8], in the fragment layout of mlp_fused16_kernel
        // (16 x 16 x 32 MFMA: large calls), and (C = 64) in that of mlp_fused_kernel (32 x 32 x 16 MFMA: small calls)
        std::vector<uint16_t *> mlp16_pk, mlp_pk;
        std::vector<uint16_t *> qkv_pk;             // register-resident LN+QKV: per layer [tile][k-step][plane][lane][8] of c_attn.weight
        std::vector<uint16_t *> proj_pk;            // FAM_REGISTER: out-projection slices per head for attn_block_kernel, [head][out tile][kk][plane][lane][8]
        struct C160 {       // C = 160: attn160o_kernel's stream per layer (c_attn * ln_1 | c_proj), its 1 / scale and spill slab (large calls);
            std::vector<uint16_t *> attn160o_pk, mlp160_pk;   // mlp160p_kernel's cyclic stream per layer and the scale c_fc * ln_2 was packed with (small calls)
            std::vector<float> attn160_inv, mlp160_inv1;
            unsigned char *attn160o_spill = nullptr;
        } c160;
        // small launches (rows <= kSmallRows: one environment, BASELINE cfg1): attn_block_kernel<HP> runs one workgroup per (row, head) and leaves the
        // heads' c_proj contributions here, [n_head][kSmallRows * 256 * C] fp32 in x's layout.  Allocated by the first small launch (Chunk::ensure_head_parts)
        float *head_parts = nullptr;
    } rg;
    struct Last1 { float *wt = nullptr; } last1;   // build_last1 (facts.last1()): attn_last1_kernel's fp32 transposes of W_q, W_v, c_proj.weight, c_fc.weight, mlp.c_proj.weight
    struct Packed {         // build_packed (facts.pk_gemm()): weights as MFMA-fragment streams [row tile][k-step][plane][lane][8], activations produced in the same layout
        std::vector<uint16_t *> attn_pk2, proj_pk2, fc_pk2, proj2_pk2;
        uint16_t *apk = nullptr;                   // FAM_PACKED: LayerNorm'ed rows in PK layout, [M/32][C/16][NP][512]
        struct Folded {     // facts.ln_fold: apk holds the RAW rows, written by the residual epilogues; W * ln.weight packings, their column sums, ...
            std::vector<uint16_t *> attn_pk2g, fc_pk2g;
            std::vector<float *> attn_cs, fc_cs;
            float2 *ln_parts = nullptr;            // ... the epilogues' partial row sums, [C / 128][M]
            float *ln_mean = nullptr;              // [M]: the mean of every row at its latest LayerNorm = the shift of its operand planes (GemmArgs::shift)
        } fold;
    } pk;
    struct Workspace {      // build_workspace (every family; sized for max_rows)
        float *x_last = nullptr;                   // last-layer shortcut: new residual rows of token 255 only, [round_up(max_rows, 256)][C] fp32
        float *x_head = nullptr;                   // x_tiled: the last-token rows in plain row-major order for the head kernel
        uint16_t *y_last = nullptr;                // pk_gemm: attention output of token 255 of every row, PK planes [rows_pad][C]
        float2 *stats = nullptr;
        uint16_t *qk[2] = {nullptr, nullptr}, *vt[2] = {nullptr, nullptr};      // per plane: [2 (q,k)][M][C]; [M][C]
        uint16_t *y[2] = {nullptr, nullptr}, *hbuf[2] = {nullptr, nullptr};     // [M][C]; [M][4C]
    } ws;
    DeviceArena mem;                               // owns every device pointer of the mode (head_parts, allocated late, included): free_mode
};

struct FastState {
    ModeState mode[3];      // indexed by MGPT_PREC_* (slot 0 unused)
};

float pick_scale(const float *h_w, size_t n, bool f16)
{
    if (!f16) return 1.0f;                       // bf16 has the fp32 exponent range
    float mx = 0.f;
    for (size_t i = 0; i < n; i++) mx = std::max(mx, fabsf(h_w[i]));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.0f;
    int e = (int)floorf(log2f(4096.0f / mx));    // largest |w| lands in [2048, 4096]: hi AND lo parts stay normal fp16
    e = std::max(-8, std::min(e, 20));
    return ldexpf(1.0f, e);
}

// power-of-two scale of W * gain: the streams that carry a weight [n / C][C] (at w_off) with the LayerNorm gain (at g_off) folded into its
// columns (c_attn.weight * ln_1.weight, c_fc.weight * ln_2.weight: model.py:19-20, 50, 86) have a scale of their own
float folded_scale(const std::vector<float> &host, size_t w_off, size_t g_off, size_t n, size_t C, bool f16)
{
    std::vector<float> wg(n);
    for (size_t i = 0; i < n; i++) wg[i] = host[w_off + i] * host[g_off + i % C];
    return pick_scale(wg.data(), n, f16);
}

// (position, token) rows for layer 0 (attn256q_kernel<.., EMB>, attn160o_kernel<.., EMB>); one per checkpoint, shared by the modes
int ensure_embed_table(mgpt_gpt *g)
{
    if (g->embed_table != nullptr) return MGPT_OK;
    const size_t C = g->C;
    MGPT_HIP(g->embed_mem.alloc(&g->embed_table, (size_t)kT * kV * C * sizeof(float)));
    hipLaunchKernelGGL(fastk::embed_table_kernel, dim3((unsigned)cdiv64((int64_t)kT * kV * (C / 4), 256)), dim3(256), 0, nullptr,
                       g->params + g->off_wte, g->params + g->off_wpe, g->embed_table, C, kV);
    MGPT_LAUNCH_CHECK();
    return MGPT_OK;
}

// the same limit of dynamic LDS for several kernels
template <class... K>
hipError_t set_max_lds_each(int bytes, K *...kernels)
{
    hipError_t e = hipSuccess;
    ((e = (e == hipSuccess) ? set_max_lds(kernels, bytes) : e), ...);
    return e;
}

// Builds one precision mode: packs the weights into the layouts of the family's kernels, raises those kernels' LDS limits and sizes the
// workspace.  Everything is allocated from m->mem, in the order of build(); a failed build is undone by free_mode (gpt_fast_forward).
template <class T, int NP>
struct ModeBuilder {
    mgpt_gpt *g;
    ModeState *m;
    const bool f16;
    const ModeFacts &f = m->facts;              // filled first by build(): the parts read it and derive nothing themselves
    const size_t C = g->C;
    const int L = g->L;
    const float *P = g->params;
    std::vector<float> host = std::vector<float>(g->n_params);      // the parameters, for the scales

    int pack_matrix(const float *d_w, size_t n_elem, float scale, PlaneSet *out)
    {
        MGPT_HIP(m->mem.alloc(&out->hi, n_elem * sizeof(uint16_t)));
        if (NP == 2) MGPT_HIP(m->mem.alloc(&out->lo, n_elem * sizeof(uint16_t)));
        out->inv_scale = 1.0f / scale;
        const int64_t n4 = (int64_t)(n_elem / 4);
        ProfScope ps(P_PACK, nullptr);
        hipLaunchKernelGGL((fastk::pack_planes_kernel<T, NP>), dim3((unsigned)cdiv64(n4, 256)), dim3(256), 0, nullptr, d_w, out->hi,
                           out->lo, n4, scale);
        MGPT_LAUNCH_CHECK();
        return MGPT_OK;
    }

    // One packed stream of n16 halves per layer that carries a weight with the LayerNorm gain folded in (of_attn: c_attn.weight * ln_1.weight,
    // else c_fc.weight * ln_2.weight): allocates it, picks the folded scale, keeps 1 / scale and packs -- launch(layer offsets, layer, stream, scale)
    template <class Launch>
    int pack_folded(std::vector<uint16_t *> &pk, std::vector<float> &inv, size_t n16, bool of_attn, Launch launch)
    {
        pk.assign(L, nullptr);
        inv.assign(L, 1.f);
        for (int l = 0; l < L; l++) {
            MGPT_HIP(m->mem.alloc(&pk[l], n16 * sizeof(uint16_t)));
            const LayerOff &lo = g->layers[l];
            const float sc = of_attn ? folded_scale(host, lo.attn_w, lo.ln1, 3 * C * C, C, f16) : folded_scale(host, lo.fc_w, lo.ln2, 4 * C * C, C, f16);
            inv[l] = 1.0f / sc;
            ProfScope ps(P_PACK, nullptr);
            launch(lo, l, pk[l], sc);
            MGPT_LAUNCH_CHECK();
        }
        return MGPT_OK;
    }

    // ---- every family: the row-major planes of the four matrices of a layer, the Phi table of the GELU epilogues ----
    int build_planes()
    {
        MGPT_HIP(hipMemcpy(host.data(), P, g->n_params * sizeof(float), hipMemcpyDeviceToHost));
        m->pl.attn.resize(L); m->pl.proj.resize(L); m->pl.fc.resize(L); m->pl.proj2.resize(L);
        int rc;
        for (int l = 0; l < L; l++) {
            const LayerOff &lo = g->layers[l];
            struct { size_t off, n; PlaneSet *dst; } mats[4] = {{lo.attn_w, 3 * C * C, &m->pl.attn[l]}, {lo.proj_w, C * C, &m->pl.proj[l]},
                                                               {lo.fc_w, 4 * C * C, &m->pl.fc[l]}, {lo.proj2_w, 4 * C * C, &m->pl.proj2[l]}};
            for (auto &mt : mats) {
                const float sc = pick_scale(host.data() + mt.off, mt.n, f16);
                if ((rc = pack_matrix(P + mt.off, mt.n, sc, mt.dst)) != MGPT_OK) return rc;
            }
        }
        // Phi(v) = (1 + erf(v / sqrt 2)) / 2 on [-6, 6) in steps of 1/256, as (value, forward difference) pairs
        std::vector<float2> lut(fastk::kGeluLutN);
        auto phi = [](double v) { return 0.5 * (1.0 + erf(v * 0.70710678118654752440)); };
        for (int i = 0; i < fastk::kGeluLutN; i++) {
            const double v0 = (i - (double)fastk::kGeluLutBias) / fastk::kGeluLutScale, v1 = (i + 1 - (double)fastk::kGeluLutBias) / fastk::kGeluLutScale;
            const float f0 = (float)phi(v0);
            lut[i] = make_float2(f0, (float)(phi(v1) - (double)f0));
        }
        MGPT_HIP(m->mem.alloc(&m->pl.gelu_lut, lut.size() * sizeof(float2)));
        MGPT_HIP(hipMemcpy(m->pl.gelu_lut, lut.data(), lut.size() * sizeof(float2), hipMemcpyHostToDevice));
        return MGPT_OK;
    }

    // ---- FAM_6M (C = 256, 8 heads of 32): MLP streams and their tables, attn256 / attn256q streams, spill slab, the layer-0 table ----
    int build_6m()
    {
        int rc;
        const size_t n16 = (size_t)fastk::kMPPeriod * 16 * NP * 512;
        m->m6.mlp256_pk.assign(L, nullptr);
        m->m6.mlp256q_pk.assign(L, nullptr);
        m->m6.mlp256_inv1.assign(L, 1.f);
        m->m6.mlp256_lut.assign(L, nullptr);
        for (int l = 0; l < L; l++) {
            MGPT_HIP(m->mem.alloc(&m->m6.mlp256_pk[l], n16 * sizeof(uint16_t)));
            MGPT_HIP(m->mem.alloc(&m->m6.mlp256q_pk[l], n16 * sizeof(uint16_t)));
            const LayerOff &lo = g->layers[l];
            const float sc1 = folded_scale(host, lo.fc_w, lo.ln2, 4 * C * C, C, f16);      // the stream carries c_fc.weight * ln_2.weight
            m->m6.mlp256_inv1[l] = 1.0f / sc1;
            {   // Phi table pre-multiplied by the (power-of-two) 1 / scale: GELU = pre-activation in stream units x entry, the same bits
                std::vector<float2> lt(fastk::kGeluLutN);
                MGPT_HIP(hipMemcpy(lt.data(), m->pl.gelu_lut, lt.size() * sizeof(float2), hipMemcpyDeviceToHost));
                for (auto &e : lt) { e.x *= m->m6.mlp256_inv1[l]; e.y *= m->m6.mlp256_inv1[l]; }
                MGPT_HIP(m->mem.alloc(&m->m6.mlp256_lut[l], lt.size() * sizeof(float2)));
                MGPT_HIP(hipMemcpy(m->m6.mlp256_lut[l], lt.data(), lt.size() * sizeof(float2), hipMemcpyHostToDevice));
            }
            ProfScope ps(P_PACK, nullptr);
            hipLaunchKernelGGL((fastk::pack_mlp256p_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)fastk::kMPPeriod * 16 * 64, 256)), dim3(256), 0,
                               nullptr, P + lo.fc_w, P + lo.proj2_w, P + lo.ln2, m->m6.mlp256_pk[l], sc1, 1.0f / m->pl.proj2[l].inv_scale);
            MGPT_LAUNCH_CHECK();
            hipLaunchKernelGGL((fastk::pack_mlp256q_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)fastk::kMPPeriod * 16 * 64, 256)), dim3(256), 0,
                               nullptr, P + lo.fc_w, P + lo.proj2_w, P + lo.ln2, m->m6.mlp256q_pk[l], sc1, 1.0f / m->pl.proj2[l].inv_scale);
            MGPT_LAUNCH_CHECK();
        }
        MGPT_HIP(set_max_lds_each(fastk::kMPLds<NP>, &fastk::mlp256p_kernel<T, NP>, &fastk::mlp256p_kernel<T, NP, 0, 2>, &fastk::mlp256q_kernel<T, NP>));
        rc = pack_folded(m->m6.attn256_pk, m->m6.attn256_inv, (size_t)8 * fastk::kA256StepsPerHead * 8 * NP * 512, true,
                         [&](const LayerOff &lo, int, uint16_t *pk, float sc) {
                             hipLaunchKernelGGL((fastk::pack_attn256_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)8 * fastk::kA256StepsPerHead * 8 * 64, 256)),
                                                dim3(256), 0, nullptr, P + lo.attn_w, P + lo.ln1, pk, sc);
                         });
        if (rc != MGPT_OK) return rc;
        // the whole attention block in one persistent kernel: 48 steps of c_attn * ln_1 followed by 16 steps of c_proj
        const size_t n16o = (size_t)fastk::kA256oPeriod * 8 * NP * 512;
        m->m6.attn256q_pk.assign(L, nullptr);
        for (int l = 0; l < L; l++) {
            const LayerOff &lo = g->layers[l];
            ProfScope ps(P_PACK, nullptr);
            MGPT_HIP(m->mem.alloc(&m->m6.attn256q_pk[l], n16o * sizeof(uint16_t)));
            hipLaunchKernelGGL((fastk::pack_attn256q_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)fastk::kA256oPeriod * 8 * 64, 256)), dim3(256), 0,
                               nullptr, P + lo.attn_w, P + lo.ln1, P + lo.proj_w, m->m6.attn256q_pk[l], 1.0f / m->m6.attn256_inv[l], 1.0f / m->pl.proj[l].inv_scale);
            MGPT_LAUNCH_CHECK();
        }
        MGPT_HIP(set_max_lds_each(fastk::kA256Lds<NP>, &fastk::attn256q_kernel<T, NP>, &fastk::attn256q_kernel<T, NP, true>));
        if ((rc = ensure_embed_table(g)) != MGPT_OK) return rc;
        MGPT_HIP(m->mem.alloc(&m->m6.attn256q_spill, (size_t)f.n_cu * 8 * 14 * NP * 1024));
        // Layer 0 of large calls from a (position, token) table of q | k | v: its input row is etab[position][token], so the row's
        // LayerNorm and q|k|v projection are a function of the pair.  The table is the output of the EMB kernel itself (TAB = 1) on kV
        // synthetic rows, row j = token j at every position: every pair in the wave, lane and MFMA slot it has in a real row, so every
        // entry is bit-identical to what layer 0 computes.  (MGPT_L0_TABLE=0 in the environment keeps the EMB kernel on layer 0.)
        if (f.l0_qkv_table) {
            ProfScope ps(P_PACK, nullptr);
            MGPT_HIP(set_max_lds_each(fastk::kA256Lds<NP>, &fastk::attn256q_kernel<T, NP, true, 1>, &fastk::attn256q_kernel<T, NP, false, 2>));
            MGPT_HIP(m->mem.alloc(&m->m6.l0_table, (size_t)kT * kV * fastk::kL0TabEntryBytes<NP>));
            DeviceArena tmp;                                 // the synthetic rows: freed on every way out, after the synchronise on the good one
            float *xt = nullptr;
            unsigned char *tk = nullptr;
            MGPT_HIP(tmp.alloc(&xt, (size_t)kV * kT * C * sizeof(float)));
            MGPT_HIP(tmp.alloc(&tk, (size_t)kV * kT));
            for (int j = 0; j < kV; j++) MGPT_HIP(hipMemset(tk + (size_t)j * kT, j, kT));
            const float scale_log2e = (1.0f / sqrtf((float)g->hs)) * 1.44269504088896340736f;    // (as forward_chunk)
            hipLaunchKernelGGL((fastk::attn256q_kernel<T, NP, true, 1>), dim3((unsigned)std::min(kV, f.n_cu)), dim3(512), (size_t)fastk::kA256Lds<NP>, nullptr, xt,
                               m->m6.attn256q_pk[0], m->m6.attn256_inv[0], scale_log2e, m->pl.proj[0].inv_scale, m->m6.attn256q_spill, kV,
                               tk, g->embed_table, m->m6.l0_table);
            MGPT_LAUNCH_CHECK();
            MGPT_HIP(hipDeviceSynchronize());
        }
        MGPT_HIP(set_max_lds(&fastk::attn256_kernel<T, NP>, fastk::kA256Lds<NP>));
        return MGPT_OK;
    }

    // ---- C = 64 / 160: the fused MLP's packets and qkv_pk, and (FAM_REGISTER: heads of 32) proj_pk and the 160-only persistent streams ----
    template <int CT>
    int build_register()
    {
        int rc;
        {
            const size_t frags = C / 16 + 2 * (C / 32), nt = 4 * C / 32;
            const size_t n16 = nt * frags * NP * 512;
            // (the small calls of C = 160 take mlp160p_kernel, below: mlp_fused_kernel's packets only for C = 64)
            if (CT == 2) m->rg.mlp_pk.assign(L, nullptr);
            m->rg.mlp16_pk.assign(L, nullptr);
            for (int l = 0; l < L; l++) {
                const LayerOff &lo = g->layers[l];
                ProfScope ps(P_PACK, nullptr);
                if (CT == 2) {
                    MGPT_HIP(m->mem.alloc(&m->rg.mlp_pk[l], n16 * sizeof(uint16_t)));
                    hipLaunchKernelGGL((fastk::pack_mlp_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)(nt * frags * 64), 256)), dim3(256), 0,
                                       nullptr, P + lo.fc_w, P + lo.proj2_w, m->rg.mlp_pk[l], (int)C, 1.0f / m->pl.fc[l].inv_scale, 1.0f / m->pl.proj2[l].inv_scale);
                    MGPT_LAUNCH_CHECK();
                }
                MGPT_HIP(m->mem.alloc(&m->rg.mlp16_pk[l], n16 * sizeof(uint16_t)));
                hipLaunchKernelGGL((fastk::pack_mlp16_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)(nt * frags * 64), 256)), dim3(256), 0,
                                   nullptr, P + lo.fc_w, P + lo.proj2_w, m->rg.mlp16_pk[l], (int)C, 1.0f / m->pl.fc[l].inv_scale, 1.0f / m->pl.proj2[l].inv_scale);
                MGPT_LAUNCH_CHECK();
            }
            const int pkt = fastk::mlp_fused_lds(NP, (int)C);
            if constexpr (CT == 2)
                MGPT_HIP(set_max_lds_each(pkt, &fastk::mlp_fused_kernel<T, NP, 2, 8>, &fastk::mlp_fused_kernel<T, NP, 2, 4>, &fastk::mlp_fused_kernel<T, NP, 2, 2>));
            MGPT_HIP(set_max_lds_each(pkt, &fastk::mlp_fused16_kernel<T, NP, CT, 8, 0>, &fastk::mlp_fused16_kernel<T, NP, CT, 4, 0>,
                                      &fastk::mlp_fused16_kernel<T, NP, CT, 2, 0>));
            if constexpr (CT == 2)                           // (C = 64 with one head of 64, FAM_GENERIC: the same kernel on plain rows)
                MGPT_HIP(set_max_lds_each(pkt, &fastk::mlp_fused16_kernel<T, NP, 2, 8, 0, 3, true>, &fastk::mlp_fused16_kernel<T, NP, 2, 4, 0, 3, true>,
                                          &fastk::mlp_fused16_kernel<T, NP, 2, 2, 0, 3, true>));
        }
        const size_t ks = C / 16, ntile = 3 * C / 32;
        m->rg.qkv_pk.assign(L, nullptr);
        for (int l = 0; l < L; l++) {
            MGPT_HIP(m->mem.alloc(&m->rg.qkv_pk[l], ntile * ks * NP * 512 * sizeof(uint16_t)));
            ProfScope ps(P_PACK, nullptr);
            hipLaunchKernelGGL((fastk::pack_rows_perm_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)(ntile * ks * 64), 256)), dim3(256), 0,
                               nullptr, P + g->layers[l].attn_w, m->rg.qkv_pk[l], (int)ntile, (int)C, 1.0f / m->pl.attn[l].inv_scale);
            MGPT_LAUNCH_CHECK();
        }
        if (f.family != FAM_REGISTER) return MGPT_OK;
        const size_t ct = C / 32;
        m->rg.proj_pk.assign(L, nullptr);
        for (int l = 0; l < L; l++) {
            MGPT_HIP(m->mem.alloc(&m->rg.proj_pk[l], (size_t)g->nh * 2 * ct * NP * 512 * sizeof(uint16_t)));
            ProfScope ps(P_PACK, nullptr);
            hipLaunchKernelGGL((fastk::pack_cols_perm_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)(g->nh * 2 * ct * 64), 256)), dim3(256), 0,
                               nullptr, P + g->layers[l].proj_w, m->rg.proj_pk[l], g->nh, (int)C, (int)C, 1.0f / m->pl.proj[l].inv_scale);
            MGPT_LAUNCH_CHECK();
        }
        // attn_block_kernel's dynamic LDS limit is a per-device function attribute: set it for this model's device
        // (C = 160 runs it in small calls only: the persistent attn160o_kernel below serves the large ones)
        const int lds = fastk::attn_block_lds(NP, (int)C);
        if constexpr (CT == 5) MGPT_HIP(set_max_lds(&fastk::attn_block_kernel<T, NP, 5, false, true>, lds));
        else MGPT_HIP(set_max_lds_each(lds, &fastk::attn_block_kernel<T, NP, 2, false, false>, &fastk::attn_block_kernel<T, NP, 2, true, false>,
                                       &fastk::attn_block_kernel<T, NP, 2, false, true>));
        // (head_parts -- the heads' partial sums of small launches -- is allocated by the first small launch: forward_chunk)
        if (CT != 5) return MGPT_OK;
        // ... and the MLP block of the small launches: mlp160p_kernel's cyclic stream per layer and the scale c_fc * ln_2 was packed with
        rc = pack_folded(m->rg.c160.mlp160_pk, m->rg.c160.mlp160_inv1, (size_t)fastk::kM5Period * 20 * NP * 512, false,
                         [&](const LayerOff &lo, int l, uint16_t *pk, float sc1) {
                             hipLaunchKernelGGL((fastk::pack_mlp160p_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)fastk::kM5Period * 20 * 64, 256)), dim3(256), 0,
                                                nullptr, P + lo.fc_w, P + lo.proj2_w, P + lo.ln2, pk, sc1, 1.0f / m->pl.proj2[l].inv_scale);
                         });
        if (rc != MGPT_OK) return rc;
        // the attention block as one persistent kernel (layers that neither gather the embedding nor are the last)
        rc = pack_folded(m->rg.c160.attn160o_pk, m->rg.c160.attn160_inv, (size_t)fastk::kA160oPeriod * fastk::kA160oFrags * NP * 512, true,
                         [&](const LayerOff &lo, int l, uint16_t *pk, float sca) {
                             hipLaunchKernelGGL((fastk::pack_attn160o_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)fastk::kA160oPeriod * fastk::kA160oFrags * 64, 256)),
                                                dim3(256), 0, nullptr, P + lo.attn_w, P + lo.ln1, P + lo.proj_w, pk, sca, 1.0f / m->pl.proj[l].inv_scale);
                         });
        if (rc != MGPT_OK) return rc;
        MGPT_HIP(m->mem.alloc(&m->rg.c160.attn160o_spill, (size_t)f.n_cu * fastk::kA160oSpillPerWg<NP>));
        MGPT_HIP(set_max_lds_each(fastk::kA160oLds<NP>, &fastk::attn160o_kernel<T, NP>, &fastk::attn160o_kernel<T, NP, true>));
        if ((rc = ensure_embed_table(g)) != MGPT_OK) return rc;
        MGPT_HIP(set_max_lds(&fastk::mlp160p_kernel<T, NP, 5>, fastk::kM5Lds<NP>));
        MGPT_HIP(set_max_lds(&fastk::mlp160p_kernel<T, NP, 5, 2>, fastk::kM5Lds<NP, 2>));
        MGPT_HIP(set_max_lds(&fastk::mlp160p_kernel<T, NP, 5, 1>, fastk::kM5Lds<NP, 1>));
        return MGPT_OK;
    }

    // ---- the last layer's attention block for token 255 alone (attn_last1_kernel): fp32 transposes of W_q, W_v and c_proj.weight, and of
    // c_fc.weight and mlp.c_proj.weight for the one-launch last layer + head of small launches ----
    template <int C_>
    int build_last1()
    {
        const LayerOff &lo = g->layers[L - 1];
        MGPT_HIP(m->mem.alloc(&m->last1.wt, (size_t)11 * C * C * sizeof(float)));
        struct { size_t off; int rows, cols; size_t dst; } mats[5] = {
            {lo.attn_w, (int)C, (int)C, 0}, {lo.attn_w + (size_t)2 * C * C, (int)C, (int)C, (size_t)C * C}, {lo.proj_w, (int)C, (int)C, (size_t)2 * C * C},
            {lo.fc_w, (int)(4 * C), (int)C, (size_t)3 * C * C}, {lo.proj2_w, (int)C, (int)(4 * C), (size_t)7 * C * C}};
        ProfScope ps(P_PACK, nullptr);
        for (const auto &mt : mats) {
            hipLaunchKernelGGL(fastk::transpose_kernel, dim3((unsigned)cdiv64((int64_t)mt.rows * mt.cols, 256)), dim3(256), 0, nullptr,
                               P + mt.off, m->last1.wt + mt.dst, mt.rows, mt.cols);
            MGPT_LAUNCH_CHECK();
        }
        MGPT_HIP(set_max_lds(&fastk::attn_last1_kernel<C_, 32, fastk::kLast1R, false>, fastk::kLast1Lds<C_, fastk::kLast1R, false>));
        if constexpr (C_ == 256) MGPT_HIP(set_max_lds(&fastk::attn_last1_kernel<C_, 32, 1, false>, fastk::kLast1Lds<C_, 1, false>));   // (Plan::last1_row_per_wg)
        MGPT_HIP(set_max_lds(&fastk::attn_last1_kernel<C_, 32, 1, true>, fastk::kLast1Lds<C_, 1, true>));
        return MGPT_OK;
    }

    // ---- facts.pk_gemm() (FAM_PACKED; FAM_6M for its out-projection): pack_pk streams, the PK4 / PK16 attributes, the LayerNorm-fold packings ----
    template <int EPI, int NWV, bool LNF, bool LUT>
    hipError_t gemm_pk_max_lds()                // gemm_pk_kernel<.., NWV, 0, LNF> (LUT: with the Phi table slot behind the ring)
    {
        return set_max_lds(&fastk::gemm_pk_kernel<T, NP, EPI, NWV, 0, LNF>, fastk::gemm_pk_lds(NP, NWV, EPI) + fastk::gemm_pk_lds_extra(LNF, LUT));
    }
    template <int EPI, int NWV, bool LNF, bool LUT>
    hipError_t gemm_pk16_max_lds()              // gemm_pk16_kernel<.., NWV, LNF>, one-plane mode only
    {
        return set_max_lds(&fastk::gemm_pk16_kernel<T, EPI, NWV, LNF>, fastk::gemm_pk_lds(NP, NWV, EPI) + fastk::gemm_pk_lds_extra(LNF, LUT));
    }
    // every (epilogue, folded LayerNorm) form with NWV waves; the residual epilogue has no folded form, the GELU one carries the Phi table
    template <int NWV>
    int gemm_pk_max_lds_all()
    {
        using namespace fastk;
        MGPT_HIP((gemm_pk_max_lds<EPI_QK, NWV, false, false>()));
        MGPT_HIP((gemm_pk_max_lds<EPI_VT, NWV, false, false>()));
        MGPT_HIP((gemm_pk_max_lds<EPI_RESID, NWV, false, false>()));
        MGPT_HIP((gemm_pk_max_lds<EPI_GELU, NWV, false, true>()));
        MGPT_HIP((gemm_pk_max_lds<EPI_QK, NWV, true, false>()));
        MGPT_HIP((gemm_pk_max_lds<EPI_VT, NWV, true, false>()));
        MGPT_HIP((gemm_pk_max_lds<EPI_GELU, NWV, true, true>()));
        if constexpr (NP == 1) {
            MGPT_HIP((gemm_pk16_max_lds<EPI_QK, NWV, false, false>()));
            MGPT_HIP((gemm_pk16_max_lds<EPI_VT, NWV, false, false>()));
            MGPT_HIP((gemm_pk16_max_lds<EPI_RESID, NWV, false, false>()));
            MGPT_HIP((gemm_pk16_max_lds<EPI_GELU, NWV, false, true>()));
            MGPT_HIP((gemm_pk16_max_lds<EPI_QK, NWV, true, false>()));
            MGPT_HIP((gemm_pk16_max_lds<EPI_VT, NWV, true, false>()));
            MGPT_HIP((gemm_pk16_max_lds<EPI_GELU, NWV, true, true>()));
        }
        return MGPT_OK;
    }

    // one matrix [R][K] at `off` as a packed-fragment stream; gain_off != 0: times the LayerNorm gain there, with its column sums in *cs
    int pack_pk(uint16_t **dst, size_t off, size_t R, size_t K, float scale, size_t gain_off = 0, float **cs = nullptr)
    {
        const float *gain = cs != nullptr ? P + gain_off : nullptr;
        MGPT_HIP(m->mem.alloc(dst, R * K * NP * sizeof(uint16_t)));
        if (cs != nullptr) MGPT_HIP(m->mem.alloc(cs, R * sizeof(float)));
        ProfScope ps(P_PACK, nullptr);
        hipLaunchKernelGGL((fastk::pack_pk_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)(R / 32) * (K / 16) * 64, 256)), dim3(256), 0,
                           nullptr, P + off, *dst, (int)R, (int)K, scale, gain);
        MGPT_LAUNCH_CHECK();
        if (cs == nullptr) return MGPT_OK;
        hipLaunchKernelGGL((fastk::colsum_pk_kernel<T, NP>), dim3((unsigned)cdiv64((int64_t)R, 256)), dim3(256), 0, nullptr, P + off,
                           gain, *cs, (int)R, (int)K, scale);
        MGPT_LAUNCH_CHECK();
        return MGPT_OK;
    }

    int build_packed()
    {
        int rc;
        m->pk.attn_pk2.assign(L, nullptr); m->pk.proj_pk2.assign(L, nullptr); m->pk.fc_pk2.assign(L, nullptr); m->pk.proj2_pk2.assign(L, nullptr);
        for (int l = 0; l < L; l++) {
            const LayerOff &lo = g->layers[l];
            if ((rc = pack_pk(&m->pk.attn_pk2[l], lo.attn_w, 3 * C, C, 1.0f / m->pl.attn[l].inv_scale)) != MGPT_OK) return rc;
            if ((rc = pack_pk(&m->pk.proj_pk2[l], lo.proj_w, C, C, 1.0f / m->pl.proj[l].inv_scale)) != MGPT_OK) return rc;
            if (f.family == FAM_PACKED) {
                if ((rc = pack_pk(&m->pk.fc_pk2[l], lo.fc_w, 4 * C, C, 1.0f / m->pl.fc[l].inv_scale)) != MGPT_OK) return rc;
                if ((rc = pack_pk(&m->pk.proj2_pk2[l], lo.proj2_w, C, 4 * C, 1.0f / m->pl.proj2[l].inv_scale)) != MGPT_OK) return rc;
            }
        }
        // 256-row tiles (8 waves), and the 128-row forms (4 waves: small calls of the C = 768 chain, the 6M shape's out-projection)
        if ((rc = gemm_pk_max_lds_all<8>()) != MGPT_OK) return rc;
        if ((rc = gemm_pk_max_lds_all<4>()) != MGPT_OK) return rc;
        if (f.family == FAM_PACKED)                          // LayerNorm planes of the GEMM chain (the 6M kernels normalise in registers)
            MGPT_HIP(m->mem.alloc(&m->pk.apk, (size_t)g->max_rows * kT * C * NP * sizeof(uint16_t)));
        // LayerNorm folded into the GEMMs (GemmArgs; mode_facts has the why): the W * ln.weight packings, their column sums, the row sums
        if (!f.ln_fold) return MGPT_OK;
        m->pk.fold.attn_pk2g.assign(L, nullptr); m->pk.fold.fc_pk2g.assign(L, nullptr); m->pk.fold.attn_cs.assign(L, nullptr); m->pk.fold.fc_cs.assign(L, nullptr);
        for (int l = 0; l < L; l++) {
            const LayerOff &lo = g->layers[l];
            if ((rc = pack_pk(&m->pk.fold.attn_pk2g[l], lo.attn_w, 3 * C, C, 1.0f / m->pl.attn[l].inv_scale, lo.ln1, &m->pk.fold.attn_cs[l])) != MGPT_OK) return rc;
            if ((rc = pack_pk(&m->pk.fold.fc_pk2g[l], lo.fc_w, 4 * C, C, 1.0f / m->pl.fc[l].inv_scale, lo.ln2, &m->pk.fold.fc_cs[l])) != MGPT_OK) return rc;
        }
        MGPT_HIP(m->mem.alloc(&m->pk.fold.ln_parts, (size_t)(C / 128) * g->max_rows * kT * sizeof(float2)));
        // (the last layer's compact launch is padded to 256 rows and addresses token 255 of each: room and finite values for all of them)
        const size_t n_mean = (size_t)((g->max_rows + 255) / 256) * 256 * kT;
        MGPT_HIP(m->mem.alloc(&m->pk.fold.ln_mean, n_mean * sizeof(float)));
        MGPT_HIP(hipMemset(m->pk.fold.ln_mean, 0, n_mean * sizeof(float)));
        return MGPT_OK;
    }

    // ---- every family: the compact last-layer rows, LayerNorm statistics, and the activation planes that are not kept on chip ----
    int build_workspace()
    {
        const size_t nl = (size_t)((g->max_rows + 255) / 256) * 256 * C;
        MGPT_HIP(m->mem.alloc(&m->ws.x_last, nl * sizeof(float)));
        MGPT_HIP(hipMemset(m->ws.x_last, 0, nl * sizeof(float)));           // padding rows stay finite
        if (f.x_tiled()) MGPT_HIP(m->mem.alloc(&m->ws.x_head, nl * sizeof(float)));
        if (f.pk_gemm()) {
            MGPT_HIP(m->mem.alloc(&m->ws.y_last, nl * NP * sizeof(uint16_t)));
            MGPT_HIP(hipMemset(m->ws.y_last, 0, nl * NP * sizeof(uint16_t)));
        }
        const size_t M = (size_t)g->max_rows * kT;
        MGPT_HIP(m->mem.alloc(&m->ws.stats, M * sizeof(float2)));
        // q|k and v^T planes exist in HBM only where the projection is a GEMM of its own: the fused attention kernels keep them on chip
        for (int p = 0; p < NP; p++) {
            if (!f.qkv_on_chip()) {
                MGPT_HIP(m->mem.alloc(&m->ws.qk[p], 2 * M * C * sizeof(uint16_t)));
                MGPT_HIP(m->mem.alloc(&m->ws.vt[p], M * C * sizeof(uint16_t)));
            }
            if (f.pk_gemm() && p > 0) continue;                                   // PK buffers interleave the planes in [0]
            MGPT_HIP(m->mem.alloc(&m->ws.y[p], M * C * (f.pk_gemm() ? NP : 1) * sizeof(uint16_t)));
            if (!f.mlp_fused) MGPT_HIP(m->mem.alloc(&m->ws.hbuf[p], 4 * M * C * (f.pk_gemm() ? NP : 1) * sizeof(uint16_t)));
        }
        return MGPT_OK;
    }

    // the facts (the device's compute units and the two environment switches are read here, once), then the family's parts in allocation order
    int build()
    {
        g->generation++;                                     // a step graph captured before this build must not be replayed as is
        int dev = 0, rc;
        hipDeviceProp_t prop;
        MGPT_HIP(hipGetDevice(&dev));
        MGPT_HIP(hipGetDeviceProperties(&prop, dev));
        auto wanted = [](const char *name) { const char *v = getenv(name); return !(v != nullptr && v[0] == '0'); };
        m->facts = mode_facts(g->C, L, g->nh, g->hs, g->max_rows, NP, std::max(1, prop.multiProcessorCount), wanted("MGPT_L0_TABLE"), wanted("MGPT_LN_FOLD"));
        if ((rc = build_planes()) != MGPT_OK) return rc;
        if (f.family == FAM_6M) rc = build_6m();
        else if (f.mlp_fused) rc = C == 160 ? build_register<5>() : build_register<2>();
        if (rc != MGPT_OK) return rc;
        if (f.last1()) rc = C == 256 ? build_last1<256>() : C == 160 ? build_last1<160>() : build_last1<64>();
        if (rc != MGPT_OK) return rc;
        if (f.pk_gemm() && (rc = build_packed()) != MGPT_OK) return rc;
        if ((rc = build_workspace()) != MGPT_OK) return rc;
        MGPT_HIP(hipDeviceSynchronize());
        m->built = true;
        return MGPT_OK;
    }
};

template <class T, int NP>
int build_mode(mgpt_gpt *g, ModeState *m, bool f16)
{
    ModeBuilder<T, NP> b = {g, m, f16};
    return b.build();
}

void free_mode(mgpt_gpt *g, ModeState *m)
{
    if (m->built) g->generation++;                       // captured step graphs hold these pointers
    m->mem.release();
    *m = ModeState();
}

// One chunk of a call: what its launches share, and the launches, each named for what it launches (forward_chunk is the sequence).
template <class T, int NP>
struct Chunk {
    mgpt_gpt *g;
    ModeState *m;
    const uint8_t *tokens;
    float *logits;              // (a sequence forward writes through seq instead)
    hipStream_t s;
    const SeqOut *seq;
    const Plan p;
    const ModeFacts &f = m->facts;
    const float *P = g->params;
    const int C = g->C, rows = p.rows, rows_pad = p.rows_pad;
    const int64_t M = p.M;
    const float scale_log2e = (1.0f / sqrtf((float)g->hs)) * 1.44269504088896340736f;

    // the GEMM chains hand one argument block per layer from launch to launch: each sets the fields it needs and clears what only it may see
    fastk::GemmArgs layer_args(int l) const
    {
        fastk::GemmArgs a = {};
        a.M = (int)M; a.C = C; a.n_head = g->nh; a.hs = g->hs; a.plane = M * C;
        a.x = g->x; a.stats = m->ws.stats; a.gain = P + g->layers[l].ln1; a.K = C;
        a.w_hi = m->pl.attn[l].hi; a.w_lo = m->pl.attn[l].lo; a.out_scale = m->pl.attn[l].inv_scale;
        a.N = 2 * C; a.o_hi = m->ws.qk[0]; a.o_lo = m->ws.qk[1];
        return a;
    }

    // head_parts is allocated by the first small launch of a context (105 MB for the 2M shape were allocated per precision mode and per
    // adapter whether or not the context ever served one environment).  New device memory: captured step graphs of this context are stale
    int ensure_head_parts()
    {
        if (!p.head_par || m->rg.head_parts != nullptr) return MGPT_OK;
        MGPT_HIP(m->mem.alloc(&m->rg.head_parts, (size_t)g->nh * (size_t)p.part_stride * sizeof(float)));
        g->generation++;
        return MGPT_OK;
    }

    int embedding()
    {
        if (p.embed == EMBED_TILED) {
            ProfScope ps(P_EMBED, s);
            hipLaunchKernelGGL(fastk::embed_tiled_kernel, dim3((unsigned)(M / 32)), dim3(256), 0, s, tokens, P + g->off_wte, P + g->off_wpe, g->x, C);
            MGPT_LAUNCH_CHECK();
        } else if (p.embed == EMBED_STATS) {
            const int rc = launch_embed_stats(tokens, P + g->off_wte, P + g->off_wpe, g->x, m->ws.stats, M, C, s);
            if (rc != MGPT_OK) return rc;
        }                                                          // (the other kinds: layer 0's attention block forms x)
        // folded LayerNorm: (mean, rstd) of the rows the next GEMM normalises live in m->ws.stats, their raw operand planes in m->pk.apk
        if (f.ln_fold)                                            // the embedding rows: the one ln_pack_kernel launch of the forward (raw mode)
            return launch_ln_pack<T, NP>(g->x, P + g->layers[0].ln1, m->pk.apk, M, C, f.x_tiled() ? 1 : 0, s, m->ws.stats, m->pk.fold.ln_mean);
        return MGPT_OK;
    }

    // (compact = the last layer's rows: token 255 of every row; their means are not needed again)
    int ln_finalize(int64_t Mrows, bool compact)
    {
        ProfScope ps(P_LAYERNORM, s);
        hipLaunchKernelGGL(fastk::ln_finalize_kernel, dim3((unsigned)cdiv64(Mrows, 256)), dim3(256), 0, s, m->pk.fold.ln_parts, C / 128, Mrows, C, m->ws.stats,
                           m->pk.fold.ln_mean, compact ? kT : 1, compact ? kT - 1 : 0, compact ? 0 : 1);
        MGPT_LAUNCH_CHECK();
        return MGPT_OK;
    }

    // ---- last layer: the attention block of token 255 alone, without K and V (attn_last1_kernel), fp32 throughout ----
    // LAST_1: -> x_last.  LAST_TAIL: one workgroup per row, and the MLP block, ln_f and the head in the same launch; logits come straight out of it
    int attn_last(int l)
    {
        const LayerOff &lo = g->layers[l];
        ProfScope ps(P_ATTN_LAST, s);
        const float *wk = P + lo.attn_w + (size_t)C * C;
#define MGPT_LAST1T(C_)                                                                                                                     \
    hipLaunchKernelGGL((fastk::attn_last1_kernel<C_, 32, 1, true>), dim3((unsigned)rows), dim3(256 * fastk::last1_split(C_)),              \
                       (size_t)(fastk::kLast1Lds<C_, 1, true>), s, g->x, P + lo.ln1, wk, m->last1.wt, (float *)nullptr, rows, scale_log2e,    \
                       P + lo.ln2, P + g->off_lnf, P + g->off_wte, logits, kV)
#define MGPT_LAST1(C_)                                                                                                                      \
    hipLaunchKernelGGL((fastk::attn_last1_kernel<C_, 32>), dim3((unsigned)(rows_pad / fastk::kLast1R)), dim3(256 * fastk::last1_split(C_)), (size_t)fastk::kLast1Lds<C_>, s, g->x, P + lo.ln1, \
                       wk, m->last1.wt, m->ws.x_last, rows, scale_log2e)
        if (p.last == LAST_TAIL) { if (C == 256) MGPT_LAST1T(256); else if (C == 160) MGPT_LAST1T(160); else MGPT_LAST1T(64); }
        else if (p.last1_row_per_wg)
            hipLaunchKernelGGL((fastk::attn_last1_kernel<256, 32, 1, false>), dim3((unsigned)rows_pad), dim3(256 * fastk::last1_split(256)),
                               (size_t)(fastk::kLast1Lds<256, 1, false>), s, g->x, P + lo.ln1, wk, m->last1.wt, m->ws.x_last, rows, scale_log2e);
        else if (C == 256) MGPT_LAST1(256); else if (C == 160) MGPT_LAST1(160); else MGPT_LAST1(64);
#undef MGPT_LAST1
#undef MGPT_LAST1T
        MGPT_LAUNCH_CHECK();
        return MGPT_OK;
    }

    // ---- the attention block of a full layer as ONE kernel (LN1, QKV, attention, out-projection, residual): q, k, v, y stay on chip ----
    int attn_block(int l)
    {
        const LayerOff &lo = g->layers[l];
        ProfScope ps(P_ATTN, s);
        const dim3 grid((unsigned)std::min(rows, f.n_cu));       // of the persistent kernels
        if (p.attn == ATTN_160O) {
            if (p.embed == EMBED_TABLE160 && l == 0)
                hipLaunchKernelGGL((fastk::attn160o_kernel<T, NP, true>), grid, dim3(512), (size_t)fastk::kA160oLds<NP>, s, g->x,
                                   m->rg.c160.attn160o_pk[l], m->rg.c160.attn160_inv[l], scale_log2e, m->pl.proj[l].inv_scale, m->rg.c160.attn160o_spill, rows, tokens, g->embed_table);
            else
                hipLaunchKernelGGL((fastk::attn160o_kernel<T, NP>), grid, dim3(512), (size_t)fastk::kA160oLds<NP>, s, g->x,
                                   m->rg.c160.attn160o_pk[l], m->rg.c160.attn160_inv[l], scale_log2e, m->pl.proj[l].inv_scale, m->rg.c160.attn160o_spill, rows);
        } else if (p.attn == ATTN_BLOCK) {
            // (C = 160 comes here in small calls only: its large calls take attn160o_kernel)
            const size_t lds = (size_t)fastk::attn_block_lds(NP, C);
#define MGPT_ATTN_BLOCK(CT_, EMB_, HP_)                                                                                                     \
    hipLaunchKernelGGL((fastk::attn_block_kernel<T, NP, CT_, EMB_, HP_>), dim3((unsigned)(HP_ ? rows * g->nh : rows)), dim3(512), lds, s, g->x, \
                       P + lo.ln1, m->rg.qkv_pk[l], m->pl.attn[l].inv_scale, m->ws.y[0], m->ws.y[1], g->nh, scale_log2e, m->rg.proj_pk[l],                  \
                       m->pl.proj[l].inv_scale, m->ws.stats, m->ws.x_last, tokens, P + g->off_wte, P + g->off_wpe, m->rg.head_parts, p.part_stride)
            if (p.head_par) { if (C == 160) MGPT_ATTN_BLOCK(5, false, true); else MGPT_ATTN_BLOCK(2, false, true); }
            else if (p.embed == EMBED_ATTN_BLOCK && l == 0) MGPT_ATTN_BLOCK(2, true, false);
            else MGPT_ATTN_BLOCK(2, false, false);
#undef MGPT_ATTN_BLOCK
        } else {
            // ATTN_256Q (gpt_kernels_c256b.h: the projection steps and the tail on v_mfma_f32_16x16x32)
            const bool emb = p.embed == EMBED_TABLE256 && l == 0;
            if (emb && p.l0_qkv_table)                               // (q | k | v of layer 0 from the (position, token) table)
                hipLaunchKernelGGL((fastk::attn256q_kernel<T, NP, false, 2>), grid, dim3(512), (size_t)fastk::kA256Lds<NP>, s, g->x,
                                   m->m6.attn256q_pk[l], m->m6.attn256_inv[l], scale_log2e, m->pl.proj[l].inv_scale, m->m6.attn256q_spill, rows,
                                   tokens, g->embed_table, m->m6.l0_table);
            else if (emb)
                hipLaunchKernelGGL((fastk::attn256q_kernel<T, NP, true>), grid, dim3(512), (size_t)fastk::kA256Lds<NP>, s, g->x,
                                   m->m6.attn256q_pk[l], m->m6.attn256_inv[l], scale_log2e, m->pl.proj[l].inv_scale, m->m6.attn256q_spill, rows,
                                   tokens, g->embed_table);
            else
                hipLaunchKernelGGL((fastk::attn256q_kernel<T, NP>), grid, dim3(512), (size_t)fastk::kA256Lds<NP>, s, g->x,
                                   m->m6.attn256q_pk[l], m->m6.attn256_inv[l], scale_log2e, m->pl.proj[l].inv_scale, m->m6.attn256q_spill, rows);
        }
        MGPT_LAUNCH_CHECK();
        return MGPT_OK;
    }

    // ---- the attention block as a chain of launches (ATTN_256_HEADS, ATTN_PACKED, ATTN_GENERIC) ----
    // LN1 + q|k and v^T projections -> planes
    int qkv_gemms(int l, fastk::GemmArgs &a)
    {
        int rc;
        if (p.attn == ATTN_GENERIC) {
            ProfScope ps(P_GEMM_QKV, s);
            if ((rc = launch_gemm16<T, NP, fastk::PRO_LN, fastk::EPI_QK>(a, C, s)) != MGPT_OK) return rc;
            a.w_hi = m->pl.attn[l].hi + (size_t)2 * C * C; a.w_lo = (NP == 2) ? m->pl.attn[l].lo + (size_t)2 * C * C : nullptr;
            a.N = C; a.o_hi = m->ws.vt[0]; a.o_lo = m->ws.vt[1];
            return launch_gemm16<T, NP, fastk::PRO_LN, fastk::EPI_VT>(a, C, s);
        }
        // (folded LayerNorm: m->pk.apk already holds the raw rows -- from the embedding or from the residual epilogue before -- and
        //  m->ws.stats their (mean, rstd); the W * ln_1.weight packing and its column sums do the rest in the epilogue)
        if (!f.ln_fold && (rc = launch_ln_pack<T, NP>(g->x, P + g->layers[l].ln1, m->pk.apk, M, C, f.x_tiled() ? 1 : 0, s)) != MGPT_OK) return rc;
        ProfScope ps(P_GEMM_QKV, s);
        const size_t tile_halves = (size_t)(C / 16) * NP * 512;          // one 32-row tile of a PK matrix with K = C
        const uint16_t *wq = f.ln_fold ? m->pk.fold.attn_pk2g[l] : m->pk.attn_pk2[l];
        a.a_hi = m->pk.apk; a.w_hi = wq; a.chunk_major = 1;
        if (f.ln_fold) { a.ln_stats = m->ws.stats; a.colsum = m->pk.fold.attn_cs[l]; }
        if ((rc = launch_gemm_pk<T, NP, fastk::EPI_QK>(a, f.n_cu, s, p.half_qkv, p.big_call)) != MGPT_OK) return rc;
        a.w_hi = wq + (size_t)(2 * C / 32) * tile_halves;                // rows 2C.. of c_attn.weight: V
        if (f.ln_fold) a.colsum = m->pk.fold.attn_cs[l] + 2 * C;
        a.N = C; a.o_hi = m->ws.vt[0]; a.o_lo = m->ws.vt[1];
        if ((rc = launch_gemm_pk<T, NP, fastk::EPI_VT>(a, f.n_cu, s, p.half_qkv, p.big_call)) != MGPT_OK) return rc;
        a.ln_stats = nullptr; a.colsum = nullptr;
        return MGPT_OK;
    }

    // ... attention -> y planes; output projection + residual (+ stats of the new rows).  last (LAST_PACKED): only token 255 of every row from here on
    int attn_chain(int l, bool last, fastk::GemmArgs &a)
    {
        const bool packed = p.attn != ATTN_GENERIC;
        int rc;
        if (p.attn == ATTN_256_HEADS) {
            // LN1 + QKV + attention, one workgroup per (row, head): q, k, v stay on chip -> y operand planes for the out-projection
            ProfScope ps(P_ATTN, s);
            hipLaunchKernelGGL((fastk::attn256_kernel<T, NP>), dim3((unsigned)rows * 8), dim3(512), (size_t)fastk::kA256Lds<NP>, s,
                               g->x, m->m6.attn256_pk[l], m->m6.attn256_inv[l], scale_log2e, m->ws.y[0]);
            MGPT_LAUNCH_CHECK();
        } else {
            if ((rc = qkv_gemms(l, a)) != MGPT_OK) return rc;
            ProfScope ps(last ? P_ATTN_LAST : P_ATTN, s);
            const uint16_t *qh = m->ws.qk[0], *ql = m->ws.qk[1], *kh = m->ws.qk[0] + M * C, *kl = (NP == 2) ? m->ws.qk[1] + M * C : nullptr;
            uint16_t *yh = last ? m->ws.y_last : m->ws.y[0];
#define MGPT_ATTN16(HS_)                                                                                                                    \
    hipLaunchKernelGGL((fastk::attn16_kernel<T, NP, HS_>), dim3(rows * g->nh), dim3(512), (size_t)fastk::attn16_lds(NP, HS_), s, qh, ql, kh, kl, \
                       m->ws.vt[0], m->ws.vt[1], yh, m->ws.y[1], g->nh, scale_log2e, packed ? 1 : 0, packed ? 1 : 0, last ? 1 : 0)
            if (g->hs == 32) MGPT_ATTN16(32); else MGPT_ATTN16(64);
#undef MGPT_ATTN16
            MGPT_LAUNCH_CHECK();
        }
        if (last) {
            ProfScope ps(P_EMBED, s);
            hipLaunchKernelGGL(fastk::gather_last_kernel, dim3((unsigned)cdiv64((int64_t)rows_pad * (C / 4), 256)), dim3(256), 0, s, g->x, m->ws.x_last, rows,
                               rows_pad, C, f.x_tiled() ? 1 : 0);
            MGPT_LAUNCH_CHECK();
        }
        a.a_hi = last ? m->ws.y_last : m->ws.y[0]; a.a_lo = m->ws.y[1]; a.K = C; a.N = C;
        a.w_hi = m->pl.proj[l].hi; a.w_lo = m->pl.proj[l].lo; a.out_scale = m->pl.proj[l].inv_scale;
        a.x_out = last ? m->ws.x_last : g->x; a.stats_out = m->ws.stats; a.x_tiled = f.x_tiled() ? 1 : 0;
        if (last) a.M = rows_pad;
        {
            ProfScope ps(last ? P_GEMM_PROJ_LAST : P_GEMM_PROJ, s);
            if (packed) {
                a.w_hi = m->pk.proj_pk2[l];
                if (f.ln_fold) {                                                      // the rows ln_2 normalises: planes + partial sums
                    a.raw_out = m->pk.apk; a.rsum_out = m->pk.fold.ln_parts;
                    a.shift = m->pk.fold.ln_mean; a.shift_stride = last ? kT : 1; a.shift_offset = last ? kT - 1 : 0;
                }
                if ((rc = launch_gemm_pk<T, NP, fastk::EPI_RESID>(a, f.n_cu, s, p.half_proj && !last, p.big_call)) != MGPT_OK) return rc;
                a.raw_out = nullptr; a.rsum_out = nullptr; a.shift = nullptr;
            } else if ((rc = launch_gemm16<T, NP, fastk::PRO_PLANES, fastk::EPI_RESID>(a, C, s)) != MGPT_OK) return rc;
        }
        if (!fused_stats(C) && !packed) return launch_row_stats(g->x, m->ws.stats, M, C, s);
        return MGPT_OK;
    }

    // ---- the MLP block in one kernel (the hidden stays in registers); last: on the compact rows of the last layer ----
    int mlp_fused(int l, bool last)
    {
        const LayerOff &lo = g->layers[l];
        float *mlp_x = last ? m->ws.x_last : g->x;
        const int64_t mlp_M = last ? (int64_t)rows_pad : M;
        ProfScope ps(last ? P_MLP_FUSED_LAST : P_MLP_FUSED, s);
        if (p.mlp == MLP_256P2 || p.mlp == MLP_256P || p.mlp == MLP_256Q) {
            // persistent: one workgroup per CU walks the 128-token blocks round-robin (results do not depend on the grid)
            const int n_blocks = (int)(mlp_M / 128);
            if (p.mlp == MLP_256P2)
                // small launch: 64-token blocks, four waves with a SIMD each (mlp256p_kernel<.., NPAIR = 2>): twice the workgroups
                hipLaunchKernelGGL((fastk::mlp256p_kernel<T, NP, 0, 2>), dim3((unsigned)std::min(2 * n_blocks, f.n_cu)), dim3(256), (size_t)fastk::kMPLds<NP>, s,
                                   mlp_x, m->m6.mlp256_pk[l], m->m6.mlp256_inv1[l], m->pl.proj2[l].inv_scale, m->m6.mlp256_lut[l], 2 * n_blocks, (unsigned long long *)nullptr);
            else if (p.mlp == MLP_256P)
                hipLaunchKernelGGL((fastk::mlp256p_kernel<T, NP>), dim3((unsigned)std::min(n_blocks, f.n_cu)), dim3(512), (size_t)fastk::kMPLds<NP>, s,
                                   mlp_x, m->m6.mlp256_pk[l], m->m6.mlp256_inv1[l], m->pl.proj2[l].inv_scale, m->m6.mlp256_lut[l], n_blocks, (unsigned long long *)nullptr);
            else
                hipLaunchKernelGGL((fastk::mlp256q_kernel<T, NP>), dim3((unsigned)std::min(n_blocks, f.n_cu)), dim3(512), (size_t)fastk::kMPLds<NP>, s,
                                   mlp_x, m->m6.mlp256q_pk[l], m->m6.mlp256_inv1[l], m->pl.proj2[l].inv_scale, m->m6.mlp256_lut[l], n_blocks, (unsigned long long *)nullptr);
        } else if (p.mlp == MLP_160P) {
            // small launch: persistent producer / consumer blocks of TOK_ tokens; the heads' partial sums are folded in
#define MGPT_MLP160P(TOK_, ...)                                                                                                             \
    hipLaunchKernelGGL((fastk::mlp160p_kernel<T, NP, __VA_ARGS__>), dim3((unsigned)std::min((int)(mlp_M / TOK_), f.n_cu)), dim3(4 * TOK_),   \
                       (size_t)(fastk::kM5Lds<NP, TOK_ / 32>), s, mlp_x, m->rg.c160.mlp160_pk[l], m->rg.c160.mlp160_inv1[l], m->pl.proj2[l].inv_scale, m->pl.gelu_lut, \
                       (int)(mlp_M / TOK_), m->rg.head_parts, p.part_stride)
            if (p.mlp160_tokens == 32) MGPT_MLP160P(32, 5, 1); else if (p.mlp160_tokens == 64) MGPT_MLP160P(64, 5, 2); else MGPT_MLP160P(128, 5);
#undef MGPT_MLP160P
        } else {
            const size_t lds = (size_t)fastk::mlp_fused_lds(NP, C);
            // 32 tokens per wave whatever the block size: small launches (cfg1: 32 rows = 32 blocks of 256 tokens) take fewer waves per block so that the tokens
            // spread over more CUs; results do not depend on the choice (one wave per workgroup is slower: 63 us per launch against 52, round 4)
#define MGPT_MLP_(CT_, NW_)                                                                                                          \
    hipLaunchKernelGGL((fastk::mlp_fused_kernel<T, NP, CT_, NW_>), dim3((unsigned)(mlp_M / (32 * NW_))), dim3(64 * NW_), lds, s, mlp_x, \
                       P + lo.ln2, m->rg.mlp_pk[l], m->pl.fc[l].inv_scale, m->pl.proj2[l].inv_scale, last ? nullptr : m->ws.stats, (int)mlp_M, m->pl.gelu_lut, \
                       m->rg.head_parts, p.part_stride)
#define MGPT_MLP16_(CT_, NW_)                                                                                                        \
    hipLaunchKernelGGL((fastk::mlp_fused16_kernel<T, NP, CT_, NW_, 0>), dim3((unsigned)(mlp_M / (32 * NW_))), dim3(64 * NW_), lds, s, mlp_x, \
                       P + lo.ln2, m->rg.mlp16_pk[l], m->pl.fc[l].inv_scale, m->pl.proj2[l].inv_scale, last ? nullptr : m->ws.stats, (int)mlp_M, m->pl.gelu_lut, \
                       (const float *)nullptr, (int64_t)0)
    // (FAM_GENERIC keeps plain rows: C = 64 with one head of 64 runs the XROW form of the kernel)
#define MGPT_MLP16R_(NW_)                                                                                                             \
    hipLaunchKernelGGL((fastk::mlp_fused16_kernel<T, NP, 2, NW_, 0, 3, true>), dim3((unsigned)(mlp_M / (32 * NW_))), dim3(64 * NW_), lds, s, mlp_x, \
                       P + lo.ln2, m->rg.mlp16_pk[l], m->pl.fc[l].inv_scale, m->pl.proj2[l].inv_scale, last ? nullptr : m->ws.stats, (int)mlp_M, m->pl.gelu_lut, \
                       (const float *)nullptr, (int64_t)0)
#define MGPT_MLP(CT_, NW_) do { if (p.mlp == MLP_FUSED) MGPT_MLP_(CT_, NW_); else if (!f.x_tiled()) MGPT_MLP16R_(NW_); else MGPT_MLP16_(CT_, NW_); } while (0)
            // (MLP_FUSED: mlp_fused_kernel folds in the heads' partial sums = n_head buffers, and n_head == C / 32 for the shapes of this path;
            //  C = 160 comes here in large calls only)
            const int nw = last ? p.mlp_nw_last : p.mlp_nw;
            if (C == 160) { if (nw == 8) MGPT_MLP16_(5, 8); else if (nw == 4) MGPT_MLP16_(5, 4); else MGPT_MLP16_(5, 2); }
            else { if (nw == 8) MGPT_MLP(2, 8); else if (nw == 4) MGPT_MLP(2, 4); else MGPT_MLP(2, 2); }
#undef MGPT_MLP
#undef MGPT_MLP16R_
#undef MGPT_MLP16_
#undef MGPT_MLP_
        }
        MGPT_LAUNCH_CHECK();
        return MGPT_OK;
    }

    // ---- the MLP block of the packed chain: LN2 -> PK planes; FC + GELU -> hidden PK planes; proj2 + residual ----
    int mlp_packed(int l, bool last, fastk::GemmArgs &a)
    {
        float *mlp_x = last ? m->ws.x_last : g->x;
        const int64_t mlp_M = last ? (int64_t)rows_pad : M;
        int rc;
        if (f.ln_fold) { if ((rc = ln_finalize(mlp_M, last)) != MGPT_OK) return rc; }
        else if ((rc = launch_ln_pack<T, NP>(mlp_x, P + g->layers[l].ln2, m->pk.apk, mlp_M, C, f.x_tiled() ? 1 : 0, s)) != MGPT_OK) return rc;
        a.M = (int)mlp_M;
        a.a_hi = m->pk.apk; a.K = C; a.N = 4 * C; a.w_hi = f.ln_fold ? m->pk.fold.fc_pk2g[l] : m->pk.fc_pk2[l]; a.out_scale = m->pl.fc[l].inv_scale;
        a.o_hi = m->ws.hbuf[0]; a.o_pk = 1; a.gelu_lut = m->pl.gelu_lut;
        if (f.ln_fold) { a.ln_stats = m->ws.stats; a.colsum = m->pk.fold.fc_cs[l]; }
        {
            ProfScope ps(P_GEMM_FC, s);
            // (c_fc keeps its 256-row tiles in small calls too: 384 of them already cover the CUs, and two 4-wave workgroups per CU move 1.5 x the ring
            //  pieces per MFMA of one 8-wave workgroup -- 54.6 vs 56.5 us per launch at 32 rows)
            if ((rc = launch_gemm_pk<T, NP, fastk::EPI_GELU>(a, f.n_cu, s, false, p.big_call)) != MGPT_OK) return rc;
        }
        a.ln_stats = nullptr; a.colsum = nullptr;
        a.a_hi = m->ws.hbuf[0]; a.K = 4 * C; a.N = C; a.w_hi = m->pk.proj2_pk2[l]; a.out_scale = m->pl.proj2[l].inv_scale;
        a.x_out = mlp_x; a.stats_out = nullptr;
        const bool feeds_next = f.ln_fold && l + 1 < g->L;            // the rows the next layer's ln_1 normalises
        if (feeds_next) { a.raw_out = m->pk.apk; a.rsum_out = m->pk.fold.ln_parts; a.shift = m->pk.fold.ln_mean; a.shift_stride = 1; a.shift_offset = 0; }
        {
            ProfScope ps(P_GEMM_PROJ2, s);
            if ((rc = launch_gemm_pk<T, NP, fastk::EPI_RESID>(a, f.n_cu, s, p.half_proj2 && !last, p.big_call)) != MGPT_OK) return rc;
        }
        return feeds_next ? ln_finalize(mlp_M, false) : MGPT_OK;
    }

    // ---- ... of the generic chain: LN2 + FC + GELU -> hidden planes; MLP output projection + residual (+ stats) ----
    int mlp_generic(int l, fastk::GemmArgs &a)
    {
        int rc;
        a.x = g->x; a.stats = m->ws.stats; a.gain = P + g->layers[l].ln2; a.K = C; a.N = 4 * C;
        a.w_hi = m->pl.fc[l].hi; a.w_lo = m->pl.fc[l].lo; a.out_scale = m->pl.fc[l].inv_scale;
        a.o_hi = m->ws.hbuf[0]; a.o_lo = m->ws.hbuf[1];
        {
            ProfScope ps(P_GEMM_FC, s);
            if ((rc = launch_gemm16<T, NP, fastk::PRO_LN, fastk::EPI_GELU>(a, C, s)) != MGPT_OK) return rc;
        }
        a.a_hi = m->ws.hbuf[0]; a.a_lo = m->ws.hbuf[1]; a.K = 4 * C; a.N = C;
        a.w_hi = m->pl.proj2[l].hi; a.w_lo = m->pl.proj2[l].lo; a.out_scale = m->pl.proj2[l].inv_scale;
        a.x_out = g->x; a.stats_out = m->ws.stats;
        {
            ProfScope ps(P_GEMM_PROJ2, s);
            if ((rc = launch_gemm16<T, NP, fastk::PRO_PLANES, fastk::EPI_RESID>(a, C, s)) != MGPT_OK) return rc;
        }
        if (!fused_stats(C) && l + 1 < g->L) return launch_row_stats(g->x, m->ws.stats, M, C, s);
        return MGPT_OK;
    }

    // ---- ln_f + head on the last token of every row (a sequence forward: at every position of the full residual stream) ----
    int head()
    {
        if (seq != nullptr) return gpt_launch_head_seq(g, g->x, f.x_tiled(), rows, kT, *seq, s);
        if (f.x_tiled()) {
            {
                ProfScope ps(P_HEAD, s);
                hipLaunchKernelGGL(fastk::untile_rows_kernel, dim3((unsigned)cdiv64((int64_t)rows * (C / 4), 256)), dim3(256), 0, s, m->ws.x_last, m->ws.x_head, rows, C);
                MGPT_LAUNCH_CHECK();
            }
            return gpt_launch_head_at(g, m->ws.x_head, (int64_t)C, 0, rows, logits, s);
        }
        return gpt_launch_head(g, rows, logits, s);
    }
};

// plan -> embedding -> for each layer { attention block; MLP block } -> head
template <class T, int NP>
int forward_chunk(mgpt_gpt *g, ModeState *m, const uint8_t *d_tokens, int rows, float *d_logits, hipStream_t s, int call_rows,
                  const SeqOut *seq = nullptr)
{
    const Plan p = make_plan(m->facts, rows, call_rows, seq != nullptr);
    Chunk<T, NP> c = {g, m, d_tokens, d_logits, s, seq, p};
    int rc;
    if ((rc = c.ensure_head_parts()) != MGPT_OK) return rc;                      // (before any kernel of the chunk is enqueued)
    if ((rc = c.embedding()) != MGPT_OK) return rc;
    for (int l = 0; l < g->L; l++) {
        const bool last = p.last != LAST_NONE && l == g->L - 1;
        if (last && p.last == LAST_TAIL) return c.attn_last(l);                   // (logits and all: no head launch)
        fastk::GemmArgs a = c.layer_args(l);
        if (last && p.last == LAST_1) rc = c.attn_last(l);
        else if (p.attn == ATTN_160O || p.attn == ATTN_BLOCK || p.attn == ATTN_256Q) rc = c.attn_block(l);
        else rc = c.attn_chain(l, last, a);
        if (rc != MGPT_OK) return rc;
        if (p.mlp == MLP_PACKED) rc = c.mlp_packed(l, last, a);
        else if (p.mlp == MLP_GENERIC) rc = c.mlp_generic(l, a);
        else rc = c.mlp_fused(l, last);
        if (rc != MGPT_OK) return rc;
    }
    return c.head();
}

template <class T, int NP, int HS>
int raise_attn_lds()
{
    MGPT_HIP(set_max_lds(&fastk::attn16_kernel<T, NP, HS>, fastk::attn16_lds(NP, HS)));
    return MGPT_OK;
}

}  // namespace

// ---- entry points used by gpt.hip ----
int gpt_fast_finalize(mgpt_gpt *g)
{
    FastState *f = static_cast<FastState *>(g->fast);
    if (f) {                                             // parameters changed: planes are rebuilt lazily
        for (auto &m : f->mode) free_mode(g, &m);
        g->embed_mem.release();                          // ... and so is the (position, token) table of layer 0
        g->embed_table = nullptr;
    } else {
        g->fast = new FastState();
    }
    return MGPT_OK;
}

void gpt_fast_destroy(mgpt_gpt *g)
{
    FastState *f = static_cast<FastState *>(g->fast);
    if (!f) return;
    for (auto &m : f->mode) free_mode(g, &m);
    delete f;
    g->fast = nullptr;
    g->embed_mem.release();
    g->embed_table = nullptr;
}

int gpt_fast_forward(mgpt_gpt *g, const uint8_t *d_tokens, int rows, float *d_logits, int precision, hipStream_t s, int call_rows,
                     const SeqOut *seq)
{
    MGPT_REQUIRE(precision == MGPT_PREC_F16X3 || precision == MGPT_PREC_BF16, MGPT_ERR_ARG, "unknown precision %d", precision);
    FastState *f = static_cast<FastState *>(g->fast);
    MGPT_REQUIRE(f, MGPT_ERR_STATE, "mgpt_gpt_finalize must precede forward");
    ModeState *m = &f->mode[precision];
    if (!m->built) {                                     // first use of this precision: pack planes, size workspace
        int rc;
        if (precision == MGPT_PREC_F16X3) {
            rc = build_mode<fastk::F16T, 2>(g, m, true);
            if (rc == MGPT_OK) rc = (g->hs == 32) ? raise_attn_lds<fastk::F16T, 2, 32>() : raise_attn_lds<fastk::F16T, 2, 64>();
        } else {
            rc = build_mode<fastk::BF16T, 1>(g, m, false);
            if (rc == MGPT_OK) rc = (g->hs == 32) ? raise_attn_lds<fastk::BF16T, 1, 32>() : raise_attn_lds<fastk::BF16T, 1, 64>();
        }
        if (rc != MGPT_OK) { free_mode(g, m); return rc; }         // no half-built planes survive a failed build (e.g. out of memory)
    }
    if (precision == MGPT_PREC_F16X3) return forward_chunk<fastk::F16T, 2>(g, m, d_tokens, rows, d_logits, s, call_rows, seq);
    return forward_chunk<fastk::BF16T, 1>(g, m, d_tokens, rows, d_logits, s, call_rows, seq);
}

// test/debug: raw copy of a fast-path workspace buffer of the given precision
//   which: 0 stats(float2[M]) 1 qk hi 2 qk lo 3 vT hi 4 vT lo 5 y hi 6 y lo 7 hidden hi 8 hidden lo
int gpt_fast_debug_copy(mgpt_gpt *g, int precision, int which, void *d_out, int64_t nbytes, hipStream_t s)
{
    FastState *f = static_cast<FastState *>(g->fast);
    MGPT_REQUIRE(f && precision >= 1 && precision <= 2 && f->mode[precision].built, MGPT_ERR_STATE, "precision %d not built", precision);
    ModeState *m = &f->mode[precision];
    const void *src = nullptr;
    switch (which) {
        case 0: src = m->ws.stats; break;
        case 1: src = m->ws.qk[0]; break;
        case 2: src = m->ws.qk[1]; break;
        case 3: src = m->ws.vt[0]; break;
        case 4: src = m->ws.vt[1]; break;
        case 5: src = m->ws.y[0]; break;
        case 6: src = m->ws.y[1]; break;
        case 7: src = m->ws.hbuf[0]; break;
        case 8: src = m->ws.hbuf[1]; break;
        default: break;
    }
    MGPT_REQUIRE(src, MGPT_ERR_ARG, "which=%d has no buffer in this mode", which);
    MGPT_HIP(hipMemcpyAsync(d_out, src, (size_t)nbytes, hipMemcpyDeviceToDevice, s));
    return MGPT_OK;
}

// test/debug: event counters of the fast-path kernels (include/mapf_gpt_amd.h)
extern "C" int mgpt_gpt_debug_counter(int which, uint64_t *value, int reset)
{
    MGPT_REQUIRE(value && which == 0, MGPT_ERR_ARG, "debug counter %d does not exist", which);
    MGPT_HIP(hipDeviceSynchronize());
    unsigned long long v = 0;
    MGPT_HIP(hipMemcpyFromSymbol(&v, HIP_SYMBOL(mgpt::fastk::g_attn_fallbacks), sizeof(v)));
    *value = (uint64_t)v;
    if (reset) {
        const unsigned long long z = 0;
        MGPT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mgpt::fastk::g_attn_fallbacks), &z, sizeof(z)));
    }
    return MGPT_OK;
}
