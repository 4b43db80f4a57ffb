// plan_check.cpp <plan_expected.txt> -- the launch plan of the 16-bit forward (mapf_gpt_amd/csrc/gpt_plan.h) checked on the host:
//   (a) every cell of the table of DESIGN.md section 3.2 against an expectation written here by hand, one named case per cell;
//   (b) every Plan field over the whole grid below against plan_expected.txt, the output of the make_plan that read ModeState's
//       flags and pointers (the commit before gpt_plan.h existed; DESIGN.md section 25 says how the table was made);
//   (c) invariants of the plan and of mode_facts over the same grid.
// Built with -fsanitize=address,undefined and run as a program of its own by tests/test_plan_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../mapf_gpt_amd/csrc/gpt_plan.h"

using namespace mgpt;

namespace {

int g_fail = 0, g_cells = 0;

struct Shape { const char *name; int L, nh, C; bool vary_tab, vary_fold; };
// the models of tools/forward_digest.py and two generic ones; all pass mgpt_gpt_create (head size 32 or 64, C % 32 == 0, C <= 1024)
const Shape kTiny = {"tiny", 2, 2, 64, false, false}, k2M = {"2M", 5, 5, 160, false, false}, k6M = {"6M", 8, 8, 256, true, false},
            k85M = {"85M", 12, 12, 768, false, true}, kC256h4 = {"c256h4", 2, 4, 256, false, true}, kC512h8 = {"c512h8", 2, 8, 512, false, true},
            kC64h1 = {"c64h1", 2, 1, 64, false, false}, kC128h4 = {"c128h4", 2, 4, 128, false, false}, kC128h2 = {"c128h2", 2, 2, 128, false, false},
            kTinyL1 = {"tiny_L1", 1, 2, 64, false, false}, k2ML1 = {"2M_L1", 1, 5, 160, false, false}, k6ML1 = {"6M_L1", 1, 8, 256, true, false};
const Shape kShapes[] = {kTiny, k2M, k6M, k85M, kC256h4, kC512h8, kC64h1, kC128h4, kC128h2, kTinyL1, k2ML1, k6ML1};

struct Case { Shape s; int np, n_cu, max_rows; bool tab, fold, seq; int rows, call_rows; };

ModeFacts facts_of(const Case &c) { return mode_facts(c.s.C, c.s.L, c.s.nh, c.s.C / c.s.nh, c.max_rows, c.np, c.n_cu, c.tab, c.fold); }

// the grid: shapes x planes x compute units x row capacity x (6M: table wanted or not) x (packed chain: fold wanted or not) x seq x
// (rows, call_rows): one row, the small-call limit and one above, the remainder chunks of a 200-row call in chunks of 128, and every
// threshold the plan has in units of compute units (MLP block sizes, wave counts, last1_row_per_wg), with one row above each
template <class F>
void for_each_case(F fn)
{
    for (const Shape &s : kShapes)
        for (int np : {1, 2})
            for (int n_cu : {256, 8})
                for (int max_rows : {128, 4096})
                    for (int tab = s.vary_tab ? 0 : 1; tab < 2; tab++)
                        for (int fold = s.vary_fold ? 0 : 1; fold < 2; fold++)
                            for (int seq = 0; seq < 2; seq++) {
                                const int pairs[][2] = {{1, 1}, {128, 128}, {129, 129}, {72, 200}, {128, 200}};
                                for (const auto &rc : pairs) fn(Case{s, np, n_cu, max_rows, tab != 0, fold != 0, seq != 0, rc[0], rc[1]});
                                for (int t : {n_cu / 8, n_cu / 4, n_cu / 2, n_cu, 2 * n_cu})
                                    for (int r : {t, t + 1}) fn(Case{s, np, n_cu, max_rows, tab != 0, fold != 0, seq != 0, r, r});
                            }
}

void print_case(FILE *o, const Case &c)
{
    fprintf(o, "%s np=%d n_cu=%d max_rows=%d tab=%d fold=%d seq=%d rows=%d/%d", c.s.name, c.np, c.n_cu, c.max_rows, c.tab, c.fold, c.seq, c.rows, c.call_rows);
}

// the table's lines: one "@ ..." line per group of kPairs (rows, call_rows) pairs, then per case the call's rows and every Plan field in
// declaration order, the one-digit fields written together; a group whose lines an earlier group has already is "@ group = earlier group"
constexpr int kPairs = 15;
void print_group(char *buf, size_t n, const Case &c)
{
    snprintf(buf, n, "@ %s np=%d n_cu=%d max_rows=%d tab=%d fold=%d seq=%d", c.s.name, c.np, c.n_cu, c.max_rows, c.tab, c.fold, c.seq);
}
void print_line(char *buf, size_t n, const Case &c, const Plan &p)
{
    snprintf(buf, n, "%d: %d %d %lld %d%d%d%d%d%d%d %lld %d%d%d %d %d%d %d%d%d", c.call_rows, p.rows, p.rows_pad, (long long)p.M, p.small, p.big_call,
             (int)p.family, (int)p.embed, p.l0_qkv_table, (int)p.attn, p.head_par, (long long)p.part_stride, (int)p.last, p.last1_row_per_wg,
             (int)p.mlp, p.mlp160_tokens, p.mlp_nw, p.mlp_nw_last, p.half_qkv, p.half_proj, p.half_proj2);
}

#define CELL(name, cond)                                                             \
    do {                                                                             \
        g_cells++;                                                                   \
        if (!(cond)) { g_fail++; printf("FAIL cell %s: %s\n", name, #cond); }      \
    } while (0)

// (a) the table of section 3.2; 256 compute units, room for 4096 rows, both switches at their defaults unless said
Plan plan(const Shape &s, int np, int rows, int call_rows, bool seq = false, bool tab = true, bool fold = true, int n_cu = 256)
{
    return make_plan(mode_facts(s.C, s.L, s.nh, s.C / s.nh, 4096, np, n_cu, tab, fold), rows, call_rows, seq);
}

void check_cells()
{
    Plan p = plan(k2M, 2, 40, 40);
    CELL("2M small: family, embedding", p.family == FAM_REGISTER && p.small && !p.big_call && p.embed == EMBED_TILED);
    CELL("2M small: attention per (row, head)", p.attn == ATTN_BLOCK && p.head_par && p.part_stride == (int64_t)128 * 256 * 160);
    CELL("2M small: MLP, 64-token blocks above 32 x CUs tokens", p.mlp == MLP_160P && p.mlp160_tokens == 64);
    CELL("2M small: one-launch last layer", p.last == LAST_TAIL);
    CELL("2M 32 rows: 32-token blocks", plan(k2M, 2, 32, 32).mlp160_tokens == 32);
    CELL("2M 128 rows: 128-token blocks", plan(k2M, 2, 128, 128).mlp160_tokens == 128);
    p = plan(kTiny, 2, 40, 40);
    CELL("tiny small: embedding, attention", p.family == FAM_REGISTER && p.embed == EMBED_TILED && p.attn == ATTN_BLOCK && p.head_par);
    CELL("tiny small: MLP with 2 waves, tail", p.mlp == MLP_FUSED && p.mlp_nw == 2 && p.last == LAST_TAIL);
    CELL("tiny 128 rows: 4 waves from 128 x CUs tokens", plan(kTiny, 2, 128, 128).mlp_nw == 4);
    p = plan(k2M, 2, 200, 200);
    CELL("2M large: table embedding, persistent attention", p.embed == EMBED_TABLE160 && p.attn == ATTN_160O && !p.head_par && !p.small && p.big_call);
    CELL("2M large: MLP waves", p.mlp == MLP_FUSED16 && p.mlp_nw == 4 && p.mlp_nw_last == 2);
    CELL("2M large: last layer", p.last == LAST_1 && !p.last1_row_per_wg);
    CELL("2M 256 rows: 8 waves from 256 x CUs tokens", plan(k2M, 2, 256, 256).mlp_nw == 8);
    p = plan(kTiny, 2, 200, 200);
    CELL("tiny large: attention block gathers", p.embed == EMBED_ATTN_BLOCK && p.attn == ATTN_BLOCK && !p.head_par);
    CELL("tiny large: MLP, last layer", p.mlp == MLP_FUSED16 && p.last == LAST_1);
    p = plan(k6M, 2, 40, 40);
    CELL("6M small: embedding, attention per (row, head), 128-row out-projection", p.family == FAM_6M && p.embed == EMBED_TILED && p.attn == ATTN_256_HEADS && p.half_proj && !p.half_qkv && !p.half_proj2);
    CELL("6M small: 64-token MLP blocks while they fit the CUs, tail", p.mlp == MLP_256P2 && p.last == LAST_TAIL && !p.head_par);
    CELL("6M 128 rows: 128-token MLP blocks", plan(k6M, 2, 128, 128).mlp == MLP_256P);
    p = plan(k6M, 2, 160, 160);
    CELL("6M large, table on", p.embed == EMBED_TABLE256 && p.l0_qkv_table && p.attn == ATTN_256Q && p.mlp == MLP_256Q && p.last == LAST_1 && !p.half_proj);
    CELL("6M large: one row per workgroup up to 2 x CUs rows", p.last1_row_per_wg && plan(k6M, 2, 512, 512).last1_row_per_wg && !plan(k6M, 2, 513, 513).last1_row_per_wg);
    p = plan(k6M, 2, 160, 160, false, false);
    CELL("6M large, table off", p.embed == EMBED_TABLE256 && !p.l0_qkv_table && p.attn == ATTN_256Q);
    for (int np : {1, 2}) {
        p = plan(k85M, np, 40, 40);
        CELL("85M small: chain", p.family == FAM_PACKED && p.embed == EMBED_TILED && p.attn == ATTN_PACKED && p.mlp == MLP_PACKED && p.last == LAST_PACKED && !p.big_call);
        CELL("85M small: 128-row tiles in one-plane mode only", p.half_qkv == (np == 1) && p.half_proj == (np == 1) && p.half_proj2 == (np == 1));
        p = plan(k85M, np, 200, 200);
        CELL("85M large: chain in 256-row tiles", p.attn == ATTN_PACKED && p.mlp == MLP_PACKED && p.last == LAST_PACKED && p.big_call && !p.half_qkv && !p.half_proj && !p.half_proj2);
    }
    CELL("85M: LayerNorm folded in one-plane mode unless switched off", mode_facts(768, 12, 12, 64, 4096, 1, 256, true, true).ln_fold &&
         !mode_facts(768, 12, 12, 64, 4096, 1, 256, true, false).ln_fold && !mode_facts(768, 12, 12, 64, 4096, 2, 256, true, true).ln_fold);
    CELL("C = 256 with heads of 64, C = 512: packed chain", plan(kC256h4, 2, 40, 40).family == FAM_PACKED && plan(kC512h8, 1, 200, 200).family == FAM_PACKED &&
         plan(kC256h4, 2, 200, 200).last == LAST_PACKED);
    for (const Shape &s : {kC128h4, kC128h2, kC64h1})
        for (int rows : {40, 200}) {
            p = plan(s, 2, rows, rows);
            CELL("generic: embedding, attention, last layer as a full layer", p.family == FAM_GENERIC && p.embed == EMBED_STATS && p.attn == ATTN_GENERIC && p.last == LAST_NONE && !p.head_par);
            CELL("generic: MLP (C = 64 with one head of 64: the fused kernel)", p.mlp == (s.C == 64 ? MLP_FUSED16 : MLP_GENERIC));
        }
    CELL("generic C = 64: facts", mode_facts(64, 2, 1, 64, 4096, 2, 256, true, true).mlp_fused && !mode_facts(64, 2, 1, 64, 4096, 2, 256, true, true).x_tiled() &&
         !mode_facts(128, 2, 4, 32, 4096, 2, 256, true, true).mlp_fused);
    for (const Shape &s : kShapes)
        for (int rows : {40, 200}) CELL("sequence forward: the last layer is a full layer", plan(s, 2, rows, rows, true).last == LAST_NONE && plan(s, 1, rows, rows, true).last == LAST_NONE);
    CELL("one layer, tiny: embedding kernel", plan(kTinyL1, 2, 200, 200).embed == EMBED_TILED && plan(kTinyL1, 2, 200, 200).last == LAST_1);
    CELL("one layer, 2M: embedding kernel", plan(k2ML1, 2, 200, 200).embed == EMBED_TILED && plan(k2ML1, 2, 200, 200).attn == ATTN_160O);
    CELL("one layer, 6M: embedding kernel, no q|k|v table", plan(k6ML1, 2, 200, 200).embed == EMBED_TILED && !plan(k6ML1, 2, 200, 200).l0_qkv_table);
    p = plan(k2M, 2, 72, 200);
    CELL("remainder chunk of a large call stays large", !p.small && p.big_call && p.attn == ATTN_160O && p.last == LAST_1 && p.rows_pad == 256 && p.M == 72 * 256);
    CELL("remainder chunk, 6M", plan(k6M, 2, 72, 200).attn == ATTN_256Q && plan(k6M, 2, 72, 200).mlp == MLP_256Q);
    CELL("8 compute units: thresholds scale", plan(k2M, 2, 1, 1, false, true, true, 8).mlp160_tokens == 32 && plan(k2M, 2, 2, 2, false, true, true, 8).mlp160_tokens == 64 &&
         plan(k2M, 2, 3, 3, false, true, true, 8).mlp160_tokens == 128 && plan(k6M, 2, 17, 17, false, true, true, 8).mlp == MLP_256P && !plan(k6M, 2, 17, 17, false, true, true, 8).last1_row_per_wg);
}

#define INV(cond)                                                                                  \
    do {                                                                                           \
        if (!(cond)) { g_fail++; printf("FAIL invariant %s: ", #cond); print_case(stdout, c); printf("\n"); } \
    } while (0)

// (c)
void check_invariants(const Case &c, const ModeFacts &f, const Plan &p)
{
    INV(!p.small || c.call_rows <= 128);
    INV(!p.head_par || f.family == FAM_REGISTER);
    INV(p.last != LAST_TAIL || (p.small && f.last1()));
    INV(p.last != LAST_PACKED || f.family == FAM_PACKED);
    INV(!c.seq || p.last == LAST_NONE);
    INV(f.family != FAM_GENERIC || (p.embed == EMBED_STATS && p.last == LAST_NONE));
    // each MLP kernel only in the family whose builder packs its stream
    INV((p.mlp == MLP_256P2 || p.mlp == MLP_256P || p.mlp == MLP_256Q) == (f.family == FAM_6M));
    INV(p.mlp != MLP_160P || (f.family == FAM_REGISTER && f.C == 160));
    INV(p.mlp != MLP_FUSED || (f.family == FAM_REGISTER && f.C == 64));
    INV(p.mlp != MLP_FUSED16 || (f.mlp_fused && (f.C == 64 || f.C == 160)));
    INV((p.mlp == MLP_PACKED) == (f.family == FAM_PACKED));
    INV(p.mlp != MLP_GENERIC || (f.family == FAM_GENERIC && !f.mlp_fused));
    INV(f.x_tiled() == (f.family != FAM_GENERIC));
    INV(p.family == f.family);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: plan_check <plan_expected.txt>\n"); return 2; }
    check_cells();
    FILE *fp = fopen(argv[1], "r");
    if (fp == nullptr) { printf("cannot open %s\n", argv[1]); return 2; }
    int n_grid = 0;
    char line[256];
    auto next_line = [&]() {                          // the next line that is no comment, without its end
        do { if (fgets(line, sizeof line, fp) == nullptr) line[0] = 0; } while (line[0] == '#');
        line[strcspn(line, "\r\n")] = 0;
    };
    std::map<std::string, std::vector<std::string>> blocks;    // group -> its kPairs lines
    const std::vector<std::string> *cur = nullptr;
    std::string group;
    size_t at = 0;
    for_each_case([&](const Case &c) {
        const ModeFacts f = facts_of(c);
        const Plan p = make_plan(f, c.rows, c.call_rows, c.seq);
        check_invariants(c, f, p);
        n_grid++;
        char want[256];
        print_group(want, sizeof want, c);
        if (group != want) {
            group = want; cur = nullptr; at = 0;
            next_line();
            const std::string l = line;
            const size_t eq = l.find(" = ");
            if (l.substr(0, eq) != group) { if (++g_fail < 20) printf("FAIL table: expected the group \"%s\", found \"%s\"\n", want, line); }
            else if (eq != std::string::npos) {
                const auto it = blocks.find("@ " + l.substr(eq + 3));
                if (it != blocks.end()) cur = &it->second;
            } else {
                std::vector<std::string> &b = blocks[group];
                for (int i = 0; i < kPairs; i++) { next_line(); b.push_back(line); }
                cur = &b;
            }
        }
        print_line(want, sizeof want, c, p);
        const char *have = (cur != nullptr && at < cur->size()) ? (*cur)[at].c_str() : "(nothing)";
        if (strcmp(have, want) != 0 && ++g_fail < 20) { printf("FAIL table: "); print_case(stdout, c); printf("\n  expected %s\n  got      %s\n", have, want); }
        at++;
    });
    char rest[512];
    while (fgets(rest, sizeof rest, fp) != nullptr)
        if (rest[0] != '#' && rest[0] != '\n') { g_fail++; printf("FAIL table: lines beyond the grid\n"); break; }
    fclose(fp);
    if (g_fail) { printf("plan_check: %d failures\n", g_fail); return 1; }
    printf("plan_check: ok (%d cells, %d grid cases)\n", g_cells, n_grid);
    return 0;
}
