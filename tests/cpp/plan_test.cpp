// Checks of the host-side plan (visual_marker_mapping_amd/csrc/plan.cpp), built from plan.cpp alone: no GPU, no HIP.
//
//   plan_test syrk K N [switch=value ...]      rank-k schedule of vmm_ba_dense_syrk's K x N product on 256 CUs
//   plan_test scene [switch=value ...] < text  plan of a scene: "n_cams n_tags n_obs" then one "cam tag" line per observation
//
// Switches are Switches fields by name (elim=cams|tags picks the eliminated family).  Every check that fails prints a
// FAIL line; the program prints the plan's decisions as "key value" lines and exits 1 after any failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../visual_marker_mapping_amd/csrc/plan.hpp"

using namespace vmm;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (g_fail++ < 20) {                                                                                       \
                printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                            \
                printf(__VA_ARGS__);                                                                                   \
                printf("\n");                                                                                          \
            }                                                                                                          \
        }                                                                                                              \
    } while (0)

static const int kCu = 256;

static bool parse_switch(Switches& s, bool& elim_cams, const char* arg)
{
    const char* eq = strchr(arg, '=');
    if (!eq)
        return false;
    const std::string k(arg, eq - arg), v(eq + 1);
    const int i = atoi(v.c_str());
    if (k == "elim") elim_cams = v == "cams";
    else if (k == "schur") s.schur = i;
    else if (k == "order_nd") s.order_nd = i != 0;
    else if (k == "order_natural") s.order_natural = i != 0;
    else if (k == "pairs") s.pairs = i;
    else if (k == "nd_leaf") s.nd_leaf = i;
    else if (k == "syrk_wide") s.syrk_wide = i != 0;
    else if (k == "syrk_no_xcd") s.syrk_no_xcd = i != 0;
    else if (k == "syrk_slices") s.syrk_slices = i;
    else if (k == "syrk_wg_per_cu") s.syrk_wg_per_cu = i;
    else return false;
    return true;
}

// ---- observation order --------------------------------------------------------------------------------------------
static void check_order(const char* name, const OrderPlan& o, int n_own, const std::vector<int32_t>& own_idx,
                        const std::vector<int32_t>& other_idx, const std::vector<double>& px)
{
    const int64_t n = (int64_t)own_idx.size();
    CHECK(o.n == n && o.n_pad >= std::max<int64_t>(n, 64) && o.n_pad % 64 == 0, "%s: sizes", name);
    std::vector<int> seen((size_t)n, 0);
    for (int64_t d = 0; d < n; ++d) {
        const int32_t c = o.caller[(size_t)d];
        CHECK(c >= 0 && c < n && seen[(size_t)c]++ == 0, "%s: caller is not a permutation at %lld", name, (long long)d);
        if (c < 0 || c >= n)
            continue;
        CHECK(o.own[(size_t)d] == own_idx[(size_t)c] && o.other[(size_t)d] == other_idx[(size_t)c], "%s: pose of %lld", name,
              (long long)d);
        for (int k = 0; k < 8; ++k)
            CHECK(o.px[(size_t)k * o.n_pad + d] == px[(size_t)8 * c + k], "%s: pixel %d of %lld", name, k, (long long)d);
        if (d > 0)   // sorted by own pose, stable
            CHECK(o.own[(size_t)d - 1] < o.own[(size_t)d]
                      || (o.own[(size_t)d - 1] == o.own[(size_t)d] && o.caller[(size_t)d - 1] < c),
                  "%s: order at %lld", name, (long long)d);
    }
    CHECK((int)o.start.size() == n_own + 1 && o.start[0] == 0 && o.start[(size_t)n_own] == n, "%s: starts", name);
    CHECK((int)o.pose_task.size() == n_own + 1 && o.pose_task[(size_t)n_own] == (int32_t)o.tasks.size(), "%s: pose_task",
          name);
    for (int p = 0; p < n_own && g_fail == 0; ++p) {
        for (int32_t d = o.start[(size_t)p]; d < o.start[(size_t)p + 1]; ++d)
            CHECK(o.own[(size_t)d] == p, "%s: run of pose %d", name, p);
        // the tasks of pose p cut its run into consecutive chunks of 1..64 observations
        int32_t at = o.start[(size_t)p];
        for (int32_t t = o.pose_task[(size_t)p]; t < o.pose_task[(size_t)p + 1]; ++t) {
            const Task& k = o.tasks[(size_t)t];
            CHECK(k.pose == p && k.begin == at && k.end > k.begin && k.end - k.begin <= kWave, "%s: task %d", name, t);
            at = k.end;
        }
        CHECK(at == o.start[(size_t)p + 1], "%s: tasks of pose %d", name, p);
    }
}

// ---- rank-k schedule ----------------------------------------------------------------------------------------------
static void check_syrk(const SyrkSchedule& s, int n_row_blk, int n_col_blk, int k_pad)
{
    CHECK(s.n_kt == k_pad / kKT, "syrk: K stages");
    std::map<std::pair<int, int>, int> tiles;
    for (int t = 0; t < s.n_tiles; ++t)
        tiles[{ s.tile_bi[(size_t)t], s.tile_bj[(size_t)t] }]++;
    int want = 0;
    for (int r = 0; r < n_row_blk; ++r)
        for (int c = 0; c <= std::min(r, n_col_blk - 1); ++c, ++want)
            CHECK(tiles[std::make_pair(r, c)] == 1, "syrk: tile (%d, %d)", r, c);
    CHECK(s.n_tiles == want && (int)tiles.size() == want, "syrk: tile count %d, want %d", s.n_tiles, want);
    CHECK((int)s.wg_u0.size() == s.n_wg && (int)s.wg_u1.size() == s.n_wg && (int)s.wg_seg0.size() == s.n_wg, "syrk: sizes");
    CHECK((int)s.tile_seg0.size() == s.n_tiles + 1 && s.tile_seg0[(size_t)s.n_tiles] == s.n_segments, "syrk: tile_seg0");
    // every (tile, K stage) unit in exactly one workgroup's range
    const int64_t n_units = (int64_t)s.n_tiles * s.n_kt;
    std::vector<int> cover((size_t)n_units, 0);
    std::vector<std::vector<std::pair<int, int>>> segs((size_t)s.n_tiles);   // per tile: (first K stage, segment)
    for (int b = 0; b < s.n_wg; ++b) {
        const int64_t u0 = s.wg_u0[(size_t)b], u1 = s.wg_u1[(size_t)b];
        CHECK(0 <= u0 && u0 <= u1 && u1 <= n_units, "syrk: range of workgroup %d", b);
        if (!(0 <= u0 && u0 <= u1 && u1 <= n_units))
            continue;
        for (int64_t u = u0; u < u1; ++u)
            cover[(size_t)u]++;
        // the workgroup's segments: one per tile its range touches, numbered from wg_seg0 in unit order
        int seg = s.wg_seg0[(size_t)b];
        for (int64_t u = u0; u < u1; ++seg) {
            const int t = (int)(u / s.n_kt);
            segs[(size_t)t].emplace_back((int)(u % s.n_kt), seg);
            u = std::min<int64_t>((int64_t)(t + 1) * s.n_kt, u1);
        }
    }
    for (int64_t u = 0; u < n_units; ++u)
        CHECK(cover[(size_t)u] == 1, "syrk: unit %lld covered %d times", (long long)u, cover[(size_t)u]);
    // a tile's segments are consecutive, from tile_seg0, in the order of their K stages
    for (int t = 0; t < s.n_tiles; ++t) {
        std::vector<std::pair<int, int>>& v = segs[(size_t)t];
        std::sort(v.begin(), v.end());
        CHECK((int)v.size() == s.tile_seg0[(size_t)t + 1] - s.tile_seg0[(size_t)t], "syrk: segments of tile %d", t);
        for (size_t i = 0; i < v.size(); ++i)
            CHECK(v[i].second == s.tile_seg0[(size_t)t] + (int)i, "syrk: segment %zu of tile %d", i, t);
    }
    printf("syrk_tiles %d\nsyrk_wg %d\nsyrk_segments %d\nsyrk_wide %d\n", s.n_tiles, s.n_wg, s.n_segments, s.wide ? 1 : 0);
}

// ---- block-sparse plan ----------------------------------------------------------------------------------------------
static void check_sparse(const Plan& P)
{
    const OrderPlan &E = P.ordE, &F = P.ordF;
    const int n_f = P.n_f;
    const bool tree = !P.h_row_of.empty();
    auto row_of = [&](int f) { return tree ? P.h_row_of[(size_t)f] : 6 * f; };
    // F-order position of every caller observation, position of an E-order observation in its kept pose's row
    std::vector<int32_t> posF((size_t)E.n);
    for (int64_t d = 0; d < F.n; ++d)
        posF[(size_t)F.caller[(size_t)d]] = (int32_t)d;
    for (int64_t d = 0; d < F.n; ++d)
        CHECK(E.caller[(size_t)P.f2e[(size_t)d]] == F.caller[(size_t)d], "f2e at %lld", (long long)d);
    auto row_pos = [&](int32_t dE) {
        const int32_t dF = posF[(size_t)E.caller[(size_t)dE]];
        return dF - F.start[(size_t)F.own[(size_t)dF]];
    };
    // pair id -> (row f1, kept pose f2 or -1 for the right-hand side)
    std::vector<int32_t> pose_at_row((size_t)P.n_pad + 6, -1);
    for (int f = 0; f < n_f; ++f)
        pose_at_row[(size_t)row_of(f)] = f;
    const size_t n_pairs = (size_t)P.pair_start[(size_t)n_f];
    std::map<std::pair<int, int>, size_t> id_of;
    std::vector<int> row_of_pair(n_pairs, -1);
    for (int f = 0; f < n_f; ++f)
        for (int32_t id = P.pair_start[(size_t)f]; id < P.pair_start[(size_t)f + 1]; ++id) {
            int f2;
            if (P.explicit_pairs) {
                const int32_t col = P.pair_col[(size_t)id];
                f2 = col < 0 ? -1 : pose_at_row[(size_t)col];
                CHECK(col < 0 || f2 >= 0, "pair %d: column %d is no kept pose's row", id, col);
            } else {
                const int j = id - P.pair_start[(size_t)f];
                f2 = j <= f ? j : -1;
            }
            CHECK(id_of.emplace(std::make_pair(f, f2), (size_t)id).second, "pair (%d, %d) listed twice", f, f2);
            row_of_pair[(size_t)id] = f;
        }
    // the terms every pair must hold: (position of the left block in row f1, E-order index of the right block) for
    // every two observations (e, f1), (e, f2) with rank(f2) <= rank(f1); the rhs pair: (position, e) per observation
    std::vector<std::vector<std::pair<int32_t, int32_t>>> want(n_pairs);
    for (int q = 0; q < P.n_e; ++q)
        for (int32_t d1 = E.start[(size_t)q]; d1 < E.start[(size_t)q + 1]; ++d1) {
            const int f1 = E.other[(size_t)d1];
            const auto rhs = id_of.find({ f1, -1 });
            CHECK(rhs != id_of.end(), "row %d has no right-hand side pair", f1);
            if (rhs != id_of.end())
                want[rhs->second].emplace_back(row_pos(d1), q);
            for (int32_t d2 = E.start[(size_t)q]; d2 < E.start[(size_t)q + 1]; ++d2) {
                const int f2 = E.other[(size_t)d2];
                if (row_of(f2) > row_of(f1))
                    continue;
                const auto it = id_of.find({ f1, f2 });
                CHECK(it != id_of.end(), "co-observed pair (%d, %d) missing", f1, f2);
                if (it != id_of.end())
                    want[it->second].emplace_back(row_pos(d1), d2);
            }
        }
    CHECK(P.pair_tstart.size() == n_pairs + 1 && P.pair_tstart[0] == 0, "pair_tstart");
    for (size_t id = 0; id < n_pairs; ++id) {
        std::vector<std::pair<int32_t, int32_t>> got;
        for (int32_t t = P.pair_tstart[id]; t < P.pair_tstart[id + 1]; ++t) {
            got.emplace_back(P.pair_terms[2 * (size_t)t], P.pair_terms[2 * (size_t)t + 1]);
            if (t > P.pair_tstart[id])
                CHECK(P.pair_terms[2 * (size_t)t - 2] <= P.pair_terms[2 * (size_t)t], "pair %zu: terms not sorted by left position",
                      id);
        }
        std::sort(got.begin(), got.end());
        std::sort(want[id].begin(), want[id].end());
        CHECK(got == want[id], "pair %zu of row %d: %zu terms, want %zu", id, row_of_pair[id], got.size(), want[id].size());
    }
    // work items: up to kPairsPerItem consecutive pairs of one row, every pair in exactly one item
    const int n_items = P.n_row_items;
    CHECK((int)P.row_items.size() == 2 * n_items, "row_items size");
    std::vector<int> cover(n_pairs, 0);
    for (int i = 0; i < n_items; ++i) {
        const int f = P.row_items[(size_t)i], p0 = P.row_items[(size_t)(n_items + i)];
        CHECK(f >= 0 && f < n_f && p0 >= P.pair_start[(size_t)f] && p0 < P.pair_start[(size_t)f + 1], "item %d", i);
        if (!(f >= 0 && f < n_f))
            continue;
        for (int p = p0; p < std::min(p0 + kPairsPerItem, P.pair_start[(size_t)f + 1]); ++p)
            cover[(size_t)p]++;
    }
    for (size_t id = 0; id < n_pairs; ++id)
        CHECK(cover[id] == 1, "pair %zu in %d work items", id, cover[id]);
    printf("pairs %zu\nterms %d\n", n_pairs, P.pair_tstart[n_pairs]);
}

// ---- tree-ordered factor --------------------------------------------------------------------------------------------
static void check_tree_factor(const Plan& P)
{
    const int nb = P.n_blk;
    auto nz = [&](int i, int k) { return (P.chol_nz[(size_t)i * kDfMaskWords + (k >> 6)] >> (k & 63)) & 1ull; };
    CHECK(P.chol_nz.size() == (size_t)(nb + 1) * kDfMaskWords, "mask size");
    // every block a co-observation (or a kept pose's own block) touches
    for (int q = 0; q < P.n_e; ++q)
        for (int32_t d1 = P.ordE.start[(size_t)q]; d1 < P.ordE.start[(size_t)q + 1]; ++d1)
            for (int32_t d2 = P.ordE.start[(size_t)q]; d2 < P.ordE.start[(size_t)q + 1]; ++d2) {
                const int r1 = P.h_row_of[(size_t)P.ordE.other[(size_t)d1]], r2 = P.h_row_of[(size_t)P.ordE.other[(size_t)d2]];
                for (int bi = r1 / kNB; bi <= (r1 + 5) / kNB; ++bi)
                    for (int bj = r2 / kNB; bj <= (r2 + 5) / kNB; ++bj)
                        CHECK(nz(std::max(bi, bj), std::min(bi, bj)), "block (%d, %d) not in the mask", bi, bj);
            }
    // closed under fill, a full diagonal and a full right-hand side row
    for (int i = 0; i < nb; ++i) {
        CHECK(nz(i, i) && nz(nb, i), "diagonal / rhs block %d", i);
        for (int k = 0; k < i; ++k)
            if (nz(i, k))
                for (int j = k + 1; j < i; ++j)
                    if (nz(j, k))
                        CHECK(nz(i, j), "fill (%d, %d) from column %d missing", i, j, k);
    }
    // panel order of block column j: exactly its non-zero k < j
    for (int j = 0; j < nb; ++j) {
        std::vector<int> ks, got;
        for (int k = 0; k < j; ++k)
            if (nz(j, k))
                ks.push_back(k);
        for (size_t q = 0; q < ks.size(); ++q)
            got.push_back(P.chol_order[(size_t)j * kDfMaxBlk + q]);
        std::sort(got.begin(), got.end());
        CHECK(got == ks, "panel order of block column %d", j);
    }
    // one workgroup and one slot per non-zero block below the diagonal and per block of the rhs row, one diagonal
    // workgroup per column, panel-major
    const int n_wg = P.n_df_wg;
    CHECK((int)P.df_wg.size() == 2 * n_wg && P.df_slot.size() == (size_t)nb * (nb + 1), "workgroup / slot sizes");
    std::map<std::pair<int, int>, int> wgs;
    for (int w = 0; w < n_wg; ++w) {
        const int j = P.df_wg[2 * (size_t)w], r = P.df_wg[2 * (size_t)w + 1];
        wgs[{ j, r }]++;
        if (w > 0)
            CHECK(P.df_wg[2 * (size_t)w - 2] <= j, "workgroup %d is not panel-major", w);
    }
    std::vector<int> slot_used(P.df_tree_slots, 0);
    for (int j = 0; j < nb; ++j) {
        CHECK(wgs[std::make_pair(j, j)] == 1, "diagonal workgroup of column %d", j);
        for (int r = j + 1; r <= nb; ++r) {
            const bool on = r == nb || nz(r, j);
            const int32_t sl = P.df_slot[(size_t)j * (nb + 1) + r];
            CHECK(wgs[std::make_pair(j, r)] == (on ? 1 : 0), "workgroups of block (%d, %d)", r, j);
            CHECK(on ? (sl >= 0 && (size_t)sl < P.df_tree_slots) : sl == -1, "slot of block (%d, %d)", r, j);
            if (on && sl >= 0 && (size_t)sl < P.df_tree_slots)
                slot_used[(size_t)sl]++;
        }
    }
    for (size_t s = 0; s < slot_used.size(); ++s)
        CHECK(slot_used[s] == 1, "slot %zu used %d times", s, slot_used[s]);
    printf("df_wg %d\n", n_wg);
}

static int run_scene(const Switches& sw, bool elim_cams)
{
    vmm_ba_problem p;
    memset(&p, 0, sizeof(p));
    long long n_obs = 0;
    if (scanf("%d %d %lld", &p.n_cams, &p.n_tags, &n_obs) != 3)
        return 2;
    p.n_obs = n_obs;
    std::vector<int32_t> cam((size_t)n_obs), tag((size_t)n_obs);
    std::vector<double> px((size_t)8 * n_obs);
    for (long long i = 0; i < n_obs; ++i)
        if (scanf("%d %d", &cam[(size_t)i], &tag[(size_t)i]) != 2)
            return 2;
    for (size_t i = 0; i < px.size(); ++i)
        px[i] = (double)i;   // any values: the order checks follow them
    p.obs_cam = cam.data();
    p.obs_tag = tag.data();
    p.obs_px = px.data();
    vmm_ba_create_options co;
    memset(&co, 0, sizeof(co));
    co.world_size = 1;
    const Plan P = make_plan(p, co, elim_cams, false, 1, false, sw);
    CHECK(P.error.empty(), "plan error: %s", P.error.c_str());
    const std::vector<int32_t>& own_e = elim_cams ? cam : tag;
    const std::vector<int32_t>& own_f = elim_cams ? tag : cam;
    check_order("E order", P.ordE, P.n_e, own_e, own_f, px);
    check_order("F order", P.ordF, P.n_f, own_f, own_e, px);
    if (P.sparse_schur) {
        check_sparse(P);
        if (!P.chol_nz.empty())
            check_tree_factor(P);
    } else {
        // the dense path's rank-k schedule (ensure_dense_schur)
        const int nr = (P.n_pad + kST) / kST, nc = (P.n_pad + kST - 1) / kST;
        check_syrk(plan_syrk(nr, nc, P.k_pad, kCu, sw), nr, nc, P.k_pad);
    }
    printf("n_e %d\nn_f %d\nsparse %d\ntree_nodes %d\nn_blk %d\nexplicit %d\n", P.n_e, P.n_f, P.sparse_schur ? 1 : 0,
           P.h_row_of.empty() ? 0 : (int)P.nd_node_first_blk.size(), P.n_blk, P.explicit_pairs ? 1 : 0);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    Switches sw;   // defaults: the tests pass every switch they want as an argument
    bool elim_cams = true;
    const bool syrk = !strcmp(argv[1], "syrk");
    const int first = syrk ? 4 : 2;
    if (syrk && argc < 4)
        return 2;
    for (int a = first; a < argc; ++a)
        if (!parse_switch(sw, elim_cams, argv[a])) {
            fprintf(stderr, "unknown argument %s\n", argv[a]);
            return 2;
        }
    if (syrk) {
        const int k = atoi(argv[2]), n = atoi(argv[3]);
        const int nb = round_up(n, kST) / kST, k_pad = round_up(k, kKT);   // as vmm_ba_dense_syrk
        check_syrk(plan_syrk(nb, nb, k_pad, kCu, sw), nb, nb, k_pad);
    } else if (strcmp(argv[1], "scene") || run_scene(sw, elim_cams)) {
        return 2;
    }
    printf("failures %d\n", g_fail);
    return g_fail ? 1 : 0;
}
