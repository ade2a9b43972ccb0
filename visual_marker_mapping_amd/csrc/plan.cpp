// Host-side plan of a bundle-adjustment handle (plan.hpp).  No HIP: what is computed here is uploaded by vmm_ba_create.
#include "plan.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>

namespace vmm {

// ---- environment switches ----------------------------------------------------------------------------------------

Switches read_switches()
{
    auto env_is = [](const char* name, char c) {
        const char* v = getenv(name);
        return v && v[0] == c;
    };
    Switches s;
    s.debug = getenv("VMM_BA_DEBUG") != nullptr;
    s.force_collectives = env_is("VMM_BA_FORCE_COLLECTIVES", '1');
    s.no_preload = env_is("VMM_BA_NO_PRELOAD", '1');   // diagnosis of the round-1 capture failure only
    s.eager_first = env_is("VMM_BA_EAGER_FIRST", '1');
    s.rccl_graph = !env_is("VMM_BA_RCCL_GRAPH", '0');
    s.use_graph = !env_is("VMM_BA_NO_GRAPH", '1');
    if (const char* v = getenv("VMM_BA_GRAPH_PASSES"))
        s.graph_passes = std::min(std::max(atoi(v), 1), 8);
    s.no_chain = env_is("VMM_BA_NO_CHAIN", '1');
    s.no_dataflow = env_is("VMM_BA_NO_DATAFLOW", '1');
    // VMM_BA_DEBUG_CAPTURE_FAIL=<rank>: that rank votes "my capture failed" although it did not
    if (const char* v = getenv("VMM_BA_DEBUG_CAPTURE_FAIL"))
        if (v[0])
            s.capture_fail_rank = atoi(v);
    // VMM_BA_DEBUG_SPIN_*: shrink the bounded spins of k_chol_dataflow / k_backsolve_chain so that they give up (tests of
    // the recovery path only).  A limit of 1 makes every wait give up at its first poll, arrived data or not: every pass
    // is then redone, deterministically.  With _WG only workgroup b of the launch gets the shrunk limit -- a give-up that
    // the other workgroups learn of through the abort word only (or not at all, when their part of the factor does not
    // depend on b's).
    if (const char* sl = getenv("VMM_BA_DEBUG_SPIN_LIMIT")) {
        const unsigned lim = (unsigned)std::max(1L, atol(sl));
        const char* sk = getenv("VMM_BA_DEBUG_SPIN_KERNEL");
        const std::string which = sk ? sk : "both";
        if (which == "df" || which == "both")
            s.spin_df = lim;
        if (which == "chain" || which == "both")
            s.spin_chain = lim;
        s.spin_once = env_is("VMM_BA_DEBUG_SPIN_ONCE", '1');
        const char* sw = getenv("VMM_BA_DEBUG_SPIN_WG");
        s.spin_wg = sw ? atoi(sw) : -1;
    }
    if (const char* v = getenv("VMM_BA_EVAL"))
        s.eval_fused = !strcmp(v, "fused");
    if (const char* v = getenv("VMM_BA_FUSED_GROUP"))
        s.fused_group = std::min(64, std::max(1, atoi(v)));
    if (const char* v = getenv("VMM_BA_SCHUR"))
        s.schur = !strcmp(v, "dense") ? 1 : !strcmp(v, "sparse") ? 2 : 0;
    if (const char* v = getenv("VMM_BA_ORDER")) {
        s.order_nd = !strcmp(v, "nd");
        s.order_natural = !strcmp(v, "natural");
    }
    if (const char* v = getenv("VMM_BA_ND_LEAF"))
        s.nd_leaf = std::max(1, atoi(v));
    if (const char* v = getenv("VMM_BA_TREE_MAX_WG"))
        s.tree_max_wg = atoi(v);
    if (const char* v = getenv("VMM_BA_TREE_MODEL"))
        s.tree_model_r3 = !strcmp(v, "r3");
    if (const char* v = getenv("VMM_BA_PAIRS"))
        s.pairs = !strcmp(v, "explicit") ? 1 : 0;
    if (const char* v = getenv("VMM_BA_SYRK_WG_PER_CU"))
        s.syrk_wg_per_cu = std::max(1, atoi(v));
    if (const char* v = getenv("VMM_BA_SYRK_SLICES"))
        s.syrk_slices = std::max(1, atoi(v));
    s.syrk_no_xcd = env_is("VMM_BA_SYRK_NO_XCD", '1');
    s.syrk_wide = !env_is("VMM_BA_SYRK_WIDE", '0');
    if (const char* v = getenv("VMM_BA_DF_MAX_WG"))
        s.df_max_wg = atoi(v);
    if (const char* v = getenv("VMM_BA_CHOL_TAIL"))
        s.chol_tail = atoi(v);
    if (const char* v = getenv("VMM_BA_DF_BULK"))
        s.df_bulk = atoi(v) > 0;
    if (const char* v = getenv("VMM_BA_DF_HELP"))
        s.df_help = v[0] == '1';
    return s;
}

// ---- point landmarks: tag pose -> its four world corners ----------------------------------------------------------
// computeMarkerCorners3D (include/visual_marker_mapping/TagReconstructor.h:33-52, called at
// src/TagReconstructor.cpp:483): R = Eigen::Quaterniond::toRotationMatrix() (no normalisation), corner = R local + t,
// corners LL, LR, UR, UL.
static void tag_to_points(const double* qt, const double* wh, double* pts)
{
    const double w = qt[0], x = qt[1], y = qt[2], z = qt[3];
    const double R[9] = { 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                          2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                          2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y) };
    static const double sx[4] = { -1.0, 1.0, 1.0, -1.0 }, sy[4] = { -1.0, -1.0, 1.0, 1.0 };
    for (int k = 0; k < 4; ++k) {
        const double lx = sx[k] * wh[0] / 2.0, ly = sy[k] * wh[1] / 2.0;
        for (int a = 0; a < 3; ++a)
            pts[3 * k + a] = (R[3 * a] * lx + R[3 * a + 1] * ly) + qt[4 + a];
    }
}

std::vector<double> pairs_from_tags(const double* tag_qt, const double* tag_wh, int n_tags)
{
    std::vector<double> pairs((size_t)14 * n_tags, 0.0);
    for (int t = 0; t < n_tags; ++t) {
        double pts[12];
        tag_to_points(tag_qt + 7 * (size_t)t, tag_wh + 2 * (size_t)t, pts);
        for (int k = 0; k < 6; ++k) {
            pairs[(size_t)14 * t + k] = pts[k];
            pairs[(size_t)14 * t + 7 + k] = pts[6 + k];
        }
    }
    return pairs;
}

// Point landmarks (doBundleAdjustment_points, src/TagReconstructor.cpp:457-644): every tag becomes its four world
// corners (:483-491), kept as two 6-dof blocks of two points each; every tag observation becomes the two corner-pair
// observations of those blocks (:549-560).
void expand_points(const vmm_ba_problem& user, PointProblem& x)
{
    const vmm_ba_problem* p = &user;
    x.tag_qt = pairs_from_tags(p->tag_qt, p->tag_wh, p->n_tags);
    x.tag_wh.assign((size_t)4 * p->n_tags, 0.0);
    x.cam.resize((size_t)2 * p->n_obs);
    x.tag.resize((size_t)2 * p->n_obs);
    x.px.assign((size_t)16 * p->n_obs, 0.0);
    for (int64_t i = 0; i < p->n_obs; ++i)
        for (int h2 = 0; h2 < 2; ++h2) {
            x.cam[(size_t)2 * i + h2] = p->obs_cam[i];
            x.tag[(size_t)2 * i + h2] = 2 * p->obs_tag[i] + h2;
            for (int k = 0; k < 4; ++k)
                x.px[(size_t)8 * (2 * i + h2) + k] = p->obs_px[8 * i + 4 * h2 + k];
        }
    x.problem = user;
    x.problem.n_tags = 2 * p->n_tags;
    x.problem.tag_qt = x.tag_qt.data();
    x.problem.tag_wh = x.tag_wh.data();
    x.problem.n_obs = 2 * p->n_obs;
    x.problem.obs_cam = x.cam.data();
    x.problem.obs_tag = x.tag.data();
    x.problem.obs_px = x.px.data();
}

// ---- observation orders --------------------------------------------------------------------------------------------

OrderPlan plan_order(int n_own, const int32_t* own_idx, const int32_t* other_idx, const double* px, int64_t n)
{
    OrderPlan o;
    std::vector<int64_t> start((size_t)n_own + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        start[own_idx[i] + 1]++;
    for (int p = 0; p < n_own; ++p)
        start[p + 1] += start[p];
    std::vector<int64_t> pos(start.begin(), start.end() - 1);
    o.n = n;
    o.n_pad = std::max<int64_t>(64, round_up(n, 64));
    o.own.resize((size_t)n);
    o.other.resize((size_t)n);
    o.caller.resize((size_t)n);
    o.px.assign((size_t)8 * o.n_pad, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t d = pos[own_idx[i]]++;
        o.own[d] = own_idx[i];
        o.other[d] = other_idx[i];
        o.caller[d] = (int32_t)i;
        for (int k = 0; k < 8; ++k)
            o.px[(size_t)k * o.n_pad + d] = px[8 * i + k];
    }
    o.pose_task.assign((size_t)n_own + 1, 0);
    for (int p = 0; p < n_own; ++p) {
        o.pose_task[p] = (int32_t)o.tasks.size();
        for (int64_t b = start[p]; b < start[p + 1]; b += kWave) {
            Task t;
            t.pose = p;
            t.begin = (int32_t)b;
            t.end = (int32_t)std::min<int64_t>(b + kWave, start[p + 1]);
            o.tasks.push_back(t);
        }
    }
    o.pose_task[n_own] = (int32_t)o.tasks.size();
    o.start.assign(start.begin(), start.end());
    return o;
}

// ---- rank-k schedule -----------------------------------------------------------------------------------------------
// Work plan of the rank-k update: lower 128x128 tiles with row blocks 0..n_row_blk-1 and column blocks
// 0..n_col_blk-1 (bj <= bi), K stages of 16 rows; the unit of work is one K stage of one tile.
//   * At most slots / 8 tiles (500 x 200: 55 tiles, 512 slots): one K slice per XCD -- workgroup b takes the
//     (b % 8)-th eighth of K of tile b / 8 (see below).
//   * Otherwise fewer tiles than workgroup slots: "stream-K" -- all units, tile-major, are cut into equal contiguous
//     ranges, one per workgroup.
//   * More tiles than slots (2000 x 1000: 1128 tiles): whole rounds of one-tile-per-workgroup first, XCD-aware:
//     workgroup b runs on XCD b % 8, so the 64 workgroups an XCD holds at a time get 64 CONSECUTIVE tiles of
//     the row-major tile list -- one or two block rows -- and sweep K in step: the A panel of a block row and
//     the B panels of its columns are fetched into that XCD's L2 once per K stage and shared (with the plain
//     stream-K order every workgroup streams its own two panels from HBM: 16 flop/B, measured HBM-bound at
//     63 TFLOP/s).  The tiles left over after the last full round are split stream-K over one more round.
// Every workgroup gets its unit range and first segment id by blockIdx; segments (one partial tile each) are
// numbered in unit order, so a tile's partials are consecutive and summed in that order.
SyrkSchedule plan_syrk(int n_row_blk, int n_col_blk, int k_pad, int n_cu, const Switches& sw)
{
    SyrkSchedule p;
    std::vector<int32_t>& bi = p.tile_bi;
    std::vector<int32_t>& bj = p.tile_bj;
    for (int r = 0; r < n_row_blk; ++r)
        for (int c = 0; c <= std::min(r, n_col_blk - 1); ++c) {
            bi.push_back(r);
            bj.push_back(c);
        }
    p.n_tiles = (int)bi.size();
    p.n_kt = k_pad / kKT;
    // two workgroups (72 KB of LDS each) per CU
    const int hw = n_cu > 0 ? n_cu : 256;
    const int per_cu = sw.syrk_wg_per_cu > 0 ? sw.syrk_wg_per_cu : 2;
    const int64_t slots = per_cu * (int64_t)hw;
    const bool xcd_rounds = !sw.syrk_no_xcd;
    const int n_xcd = 8;
    std::vector<int64_t>& wg_u0 = p.wg_u0;
    std::vector<int64_t>& wg_u1 = p.wg_u1;
    std::vector<int32_t>& wg_seg0 = p.wg_seg0;
    std::vector<int32_t>& tile_seg0 = p.tile_seg0;
    tile_seg0.assign((size_t)p.n_tiles + 1, 0);
    int seg = 0;
    if (xcd_rounds && (int64_t)p.n_tiles * n_xcd <= slots && p.n_kt >= n_xcd) {
        // Few tiles (500 x 200: 55): one K slice per XCD.  Workgroup b runs on XCD b % 8 (round-robin dispatch)
        // and owns the (b % 8)-th eighth of K of tile b / 8, so the 55 workgroups of an XCD sweep the SAME rows of
        // Z in step: every row is fetched into that XCD's L2 once and shared (Z crosses the fabric once per launch
        // instead of once per workgroup), and every tile leaves exactly eight partials.  Off-diagonal tiles come
        // first in the tile list: the second workgroup a CU receives is then one of the cheaper diagonal tiles.
        std::vector<int> order;
        for (int t = 0; t < p.n_tiles; ++t)
            if (bi[t] != bj[t])
                order.push_back(t);
        for (int t = 0; t < p.n_tiles; ++t)
            if (bi[t] == bj[t])
                order.push_back(t);
        std::vector<int32_t> bi2(bi.size()), bj2(bj.size());
        for (int t = 0; t < p.n_tiles; ++t) {
            bi2[t] = bi[order[t]];
            bj2[t] = bj[order[t]];
        }
        bi.swap(bi2);
        bj.swap(bj2);
        // Round 4: one 8-wave workgroup per CU (k_syrk_wide), one K slice of ONE tile each; a diagonal tile costs 9/16 of
        // an off-diagonal one there and gets as many fewer workgroups.  500 x 200: 45 x 5 + 10 x 3 = 255 workgroups on
        // 256 CUs, 255 partial tiles instead of 495.  VMM_BA_SYRK_WIDE=0: the two-workgroups-per-CU kernel below.
        if (sw.syrk_wide && !sw.syrk_slices && !sw.syrk_wg_per_cu) {
            int n_diag = 0;
            for (int t = 0; t < p.n_tiles; ++t)
                n_diag += bi[t] == bj[t];
            const int n_off = p.n_tiles - n_diag;
            const double kDiagCost = 9.0 / 16.0;
            const int max_w = std::max(1, p.n_kt / 2);   // at least one 32-row stage per workgroup
            int w_off = (int)std::floor(hw / (n_off + kDiagCost * n_diag));
            w_off = std::max(1, std::min(w_off, max_w));
            int w_diag = std::max(1, std::min((int)std::lround(kDiagCost * w_off), max_w));
            while (w_off > 1 && (int64_t)w_off * n_off + (int64_t)w_diag * n_diag > hw) {
                --w_off;
                w_diag = std::max(1, std::min((int)std::lround(kDiagCost * w_off), max_w));
            }
            std::vector<int> w_of((size_t)p.n_tiles);
            int n_items = 0;
            for (int t = 0; t < p.n_tiles; ++t) {
                w_of[t] = bi[t] == bj[t] ? w_diag : w_off;
                tile_seg0[t] = n_items;
                n_items += w_of[t];
            }
            tile_seg0[p.n_tiles] = n_items;
            // items slice-major (all tiles' first slices, then the second ones, ...): XCD x takes the x-th run of them, so
            // the workgroups an XCD holds sweep the same rows of Z
            std::vector<std::pair<int, int>> items;
            for (int sl = 0; sl < std::max(w_off, w_diag); ++sl)
                for (int t = 0; t < p.n_tiles; ++t)
                    if (sl < w_of[t])
                        items.emplace_back(t, sl);
            const int per_x = (n_items + n_xcd - 1) / n_xcd;
            p.n_wg = per_x * n_xcd;
            p.wide = true;
            wg_u0.assign((size_t)p.n_wg, 0);
            wg_u1.assign((size_t)p.n_wg, 0);
            wg_seg0.assign((size_t)p.n_wg, 0);
            for (int b = 0; b < p.n_wg; ++b) {
                const int x = b % n_xcd, j = b / n_xcd;
                const int it = x * per_x + j;
                if (j >= per_x || it >= n_items)
                    continue;
                const int t = items[(size_t)it].first, sl = items[(size_t)it].second;
                wg_u0[b] = (int64_t)t * p.n_kt + (int64_t)p.n_kt * sl / w_of[t];
                wg_u1[b] = (int64_t)t * p.n_kt + (int64_t)p.n_kt * (sl + 1) / w_of[t];
                wg_seg0[b] = tile_seg0[t] + sl;
            }
            seg = n_items;
        } else {
        // K slices per tile: as many as fit the workgroup slots (two per CU), so that every SIMD carries about the
        // same number of MFMAs (8 slices on 440 of 512 slots left 184 CUs with two workgroups and 72 with one)
        int n_sl = (int)std::min<int64_t>(slots / p.n_tiles, p.n_kt);
        if (sw.syrk_slices)
            n_sl = std::max(1, std::min(sw.syrk_slices, p.n_kt));
        const int n_items = p.n_tiles * n_sl;
        const int per_x = (n_items + n_xcd - 1) / n_xcd;
        p.n_wg = per_x * n_xcd;
        wg_u0.assign((size_t)p.n_wg, 0);
        wg_u1.assign((size_t)p.n_wg, 0);
        wg_seg0.assign((size_t)p.n_wg, 0);
        for (int b = 0; b < p.n_wg; ++b) {
            // items in slice-major order; XCD x (blockIdx % 8) takes the x-th run of per_x items: one or two slices of K
            const int x = b % n_xcd, j = b / n_xcd;
            const int it = x * per_x + j;
            if (j >= per_x || it >= n_items)
                continue;
            const int sl = it / p.n_tiles, t = it % p.n_tiles;
            wg_u0[b] = (int64_t)t * p.n_kt + (int64_t)p.n_kt * sl / n_sl;
            wg_u1[b] = (int64_t)t * p.n_kt + (int64_t)p.n_kt * (sl + 1) / n_sl;
            wg_seg0[b] = n_sl * t + sl;
        }
        for (int t = 0; t <= p.n_tiles; ++t)
            tile_seg0[t] = n_sl * t;
        seg = n_sl * p.n_tiles;
        }
    } else {
    const int64_t full_rounds = (xcd_rounds && slots % n_xcd == 0) ? p.n_tiles / slots : 0;
    const int64_t tiles_a = full_rounds * slots;                      // one tile per workgroup
    const int64_t units_b = (int64_t)(p.n_tiles - tiles_a) * p.n_kt;  // the rest: stream-K
    int64_t n_wg_b = std::min<int64_t>(units_b, slots);
    if (full_rounds == 0 && units_b > 64 * slots)
        n_wg_b = 4 * slots;   // xcd_rounds switched off: several waves of stream-K workgroups
    const int64_t upw_b = n_wg_b > 0 ? (units_b + n_wg_b - 1) / n_wg_b : 0;
    n_wg_b = upw_b > 0 ? (units_b + upw_b - 1) / upw_b : 0;
    p.n_wg = (int)(tiles_a + n_wg_b);
    // logical workgroup l (unit order) -> [u0, u1); segments numbered in unit order
    std::vector<int64_t> lu0((size_t)p.n_wg + 1, 0);
    for (int64_t l = 0; l < tiles_a; ++l)
        lu0[(size_t)l] = l * p.n_kt;
    for (int64_t l = 0; l <= n_wg_b; ++l)
        lu0[(size_t)(tiles_a + l)] = std::min<int64_t>(tiles_a * p.n_kt + l * upw_b, (int64_t)p.n_tiles * p.n_kt);
    std::vector<int32_t> lseg0((size_t)p.n_wg + 1, 0);
    for (int l = 0; l < p.n_wg; ++l) {
        lseg0[l] = seg;
        int64_t u = lu0[l];
        const int64_t u_end = lu0[l + 1];
        while (u < u_end) {
            const int t = (int)(u / p.n_kt);
            const int kt0 = (int)(u % p.n_kt);
            const int64_t take = std::min<int64_t>(p.n_kt - kt0, u_end - u);
            if (kt0 == 0)
                tile_seg0[t] = seg;
            u += take;
            ++seg;
        }
    }
    tile_seg0[p.n_tiles] = seg;
    // blockIdx -> logical workgroup: inside a full round, XCD x (blockIdx % 8) takes the x-th run of slots/8 tiles
    wg_u0.resize((size_t)p.n_wg);
    wg_u1.resize((size_t)p.n_wg);
    wg_seg0.resize((size_t)p.n_wg);
    for (int b = 0; b < p.n_wg; ++b) {
        int64_t l = b;
        if (b < tiles_a) {
            const int64_t r = b / slots, o = b % slots;
            l = r * slots + (o % n_xcd) * (slots / n_xcd) + o / n_xcd;
        }
        wg_u0[b] = lu0[(size_t)l];
        wg_u1[b] = lu0[(size_t)l + 1];
        wg_seg0[b] = lseg0[(size_t)l];
    }
    }
    p.n_segments = seg;
    return p;
}

// ---- block structure of the factor under a tree ordering ---------------------------------------------------------
// One mask per 64-row block row (kDfMaskWords words: up to 255 block columns), bit k = block (i, k) of the factor may be
// non-zero: the blocks the kept poses' 6x6 blocks touch (rows = first row of every kept pose, nbr = the co-observation
// graph), then symbolic fill (eliminating block column k couples every two block rows with an entry in it).  Row nb is the
// right-hand side row: all ones.
struct BlkMask {
    unsigned long long w[kDfMaskWords] = {};
    void set(int k) { w[k >> 6] |= 1ull << (k & 63); }
    bool test(int k) const { return (w[k >> 6] >> (k & 63)) & 1ull; }
};

static std::vector<BlkMask> symbolic_factor(int nb, const std::vector<int32_t>& rows,
                                            const std::vector<std::vector<int32_t>>& nbr)
{
    std::vector<BlkMask> nz((size_t)nb + 1);
    for (int i = 0; i < nb; ++i)
        nz[(size_t)i].set(i);
    const int n_f = (int)rows.size();
    auto touch = [&](int f1, int f2) {
        const int r1 = rows[(size_t)f1], r2 = rows[(size_t)f2];
        for (int bi = r1 / kNB; bi <= (r1 + 5) / kNB; ++bi)
            for (int bj = r2 / kNB; bj <= (r2 + 5) / kNB; ++bj)
                nz[(size_t)std::max(bi, bj)].set(std::min(bi, bj));
    };
    for (int fq = 0; fq < n_f; ++fq) {
        touch(fq, fq);
        for (const int32_t f2 : nbr[(size_t)fq])
            touch(fq, f2);
    }
    for (int k = 0; k < nb; ++k)
        for (int i = k + 1; i < nb; ++i)
            if (nz[(size_t)i].test(k))
                for (int j2 = k + 1; j2 <= i; ++j2)
                    if (nz[(size_t)j2].test(k))
                        nz[(size_t)i].set(j2);
    for (int k = 0; k < nb; ++k)
        nz[(size_t)nb].set(k);
    return nz;
}

// The model of the one-launch kernel the ordering decisions use (microseconds; measured in round 4: a block column's own
// eight rounds 7.1; a panel's eight slices are 8 of work for the workgroup that applies them, which it does while they are
// produced -- it is 2.7 behind when the panel ends): when block column j is done if it takes its panels in the order they
// finish.  Also fills the order and the longest chain of dependent columns.  old_model: VMM_BA_TREE_MODEL=r3.
static double model_tree_factorisation(int nb, const std::vector<BlkMask>& nz, std::vector<unsigned char>* ord, int* path_max,
                                       bool old_model)
{
    std::vector<double> t_done((size_t)nb, 0.0);
    std::vector<int> path((size_t)nb, 1);
    int pm = 0;
    for (int j2 = 0; j2 < nb; ++j2) {
        std::vector<int> ks;
        for (int k = 0; k < j2; ++k)
            if (nz[(size_t)j2].test(k))
                ks.push_back(k);
        std::stable_sort(ks.begin(), ks.end(), [&](int x, int y) { return t_done[(size_t)x] < t_done[(size_t)y]; });
        double t = 0.0;
        for (size_t q = 0; q < ks.size(); ++q) {
            if (ord)
                (*ord)[(size_t)j2 * kDfMaxBlk + q] = (unsigned char)ks[q];
            t = old_model ? std::max(t, t_done[(size_t)ks[q]]) + 5.6 : std::max(t + 8.0, t_done[(size_t)ks[q]] + 2.7);
            path[(size_t)j2] = std::max(path[(size_t)j2], path[(size_t)ks[q]] + 1);
        }
        t_done[(size_t)j2] = t + (old_model ? 11.0 : 7.1);
        pm = std::max(pm, path[(size_t)j2]);
    }
    if (path_max)
        *path_max = pm;
    double t_end = 0.0;
    for (const double t : t_done)
        t_end = std::max(t_end, t);
    return t_end;
}

// ---- tree ordering of the kept family (block-sparse path) -------------------------------------------------------
// Nested dissection of the co-observation graph of the kept poses (two kept poses are neighbours when one eliminated
// pose sees both: exactly the non-zero blocks of the reduced system).  A part is cut at the breadth-first level (from a
// pseudo-peripheral vertex) that balances the two sides; the level is the separator and is ordered BEHIND both sides,
// recursively.  `nodes` comes out in elimination order (children before their separator); parts of one level do not
// touch each other, so their block columns of the factor do not depend on each other.
static void nd_dissect(const std::vector<std::vector<int32_t>>& nbr, std::vector<int32_t> verts, int leaf_max, int depth,
                       std::vector<int32_t>& stamp, int32_t& stamp_next, std::vector<std::vector<int32_t>>& nodes)
{
    if (verts.empty())
        return;
    if ((int)verts.size() <= leaf_max || depth <= 0) {
        nodes.push_back(std::move(verts));
        return;
    }
    // connected components of the induced subgraph
    const int32_t in_set = stamp_next++;
    for (const int32_t v : verts)
        stamp[(size_t)v] = in_set;
    std::vector<std::vector<int32_t>> comps;
    {
        const int32_t seen = stamp_next++;
        for (const int32_t v0 : verts) {
            if (stamp[(size_t)v0] != in_set)
                continue;
            comps.emplace_back();
            std::vector<int32_t>& c = comps.back();
            c.push_back(v0);
            stamp[(size_t)v0] = seen;
            for (size_t h = 0; h < c.size(); ++h)
                for (const int32_t w : nbr[(size_t)c[h]])
                    if (stamp[(size_t)w] == in_set) {
                        stamp[(size_t)w] = seen;
                        c.push_back(w);
                    }
        }
    }
    if (comps.size() > 1) {
        // independent already: two groups of about equal size, no separator
        std::sort(comps.begin(), comps.end(),
                  [](const std::vector<int32_t>& a, const std::vector<int32_t>& b) { return a.size() > b.size(); });
        std::vector<int32_t> A, B;
        for (auto& c : comps) {
            std::vector<int32_t>& dst = A.size() <= B.size() ? A : B;
            dst.insert(dst.end(), c.begin(), c.end());
        }
        nd_dissect(nbr, std::move(A), leaf_max, depth - 1, stamp, stamp_next, nodes);
        nd_dissect(nbr, std::move(B), leaf_max, depth - 1, stamp, stamp_next, nodes);
        return;
    }
    // level structure from a pseudo-peripheral vertex (two sweeps)
    std::vector<int32_t> order, level_of_pos;
    int32_t root = verts[0];
    for (int sweep = 0; sweep < 2; ++sweep) {
        const int32_t mark = stamp_next++, todo = stamp_next++;
        for (const int32_t v : verts)
            stamp[(size_t)v] = todo;
        order.assign(1, root);
        level_of_pos.assign(1, 0);
        stamp[(size_t)root] = mark;
        for (size_t h = 0; h < order.size(); ++h)
            for (const int32_t w : nbr[(size_t)order[h]])
                if (stamp[(size_t)w] == todo) {
                    stamp[(size_t)w] = mark;
                    order.push_back(w);
                    level_of_pos.push_back(level_of_pos[h] + 1);
                }
        root = order.back();
    }
    const int n_levels = level_of_pos.back() + 1;
    if (n_levels < 3) {   // (nearly) complete graph: nothing to cut
        nodes.push_back(std::move(verts));
        return;
    }
    std::vector<int32_t> cnt((size_t)n_levels, 0);
    for (const int32_t l : level_of_pos)
        cnt[(size_t)l]++;
    int best = 1;
    long long best_cost = -1;
    for (int l = 1, below = cnt[0]; l + 1 < n_levels; below += cnt[(size_t)l], ++l) {
        const int above = (int)order.size() - below - cnt[(size_t)l];
        const long long cost = (long long)std::abs(below - above) * 4 + cnt[(size_t)l];
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = l;
        }
    }
    std::vector<int32_t> A, B, S;
    for (size_t h = 0; h < order.size(); ++h)
        (level_of_pos[h] < best ? A : level_of_pos[h] > best ? B : S).push_back(order[h]);
    nd_dissect(nbr, std::move(A), leaf_max, depth - 1, stamp, stamp_next, nodes);
    nd_dissect(nbr, std::move(B), leaf_max, depth - 1, stamp, stamp_next, nodes);
    nodes.push_back(std::move(S));
}

// ---- the plan of a handle ------------------------------------------------------------------------------------------

// Fused evaluation (k_eval_fused: one evaluation per observation, lane = kept pose, both families' sums in
// registers).  Opt-in, VMM_BA_EVAL=fused: it needs ~370 registers per lane, so one wave per SIMD, and measured
// SLOWER than the two-pass kernel at two waves per SIMD (500 x 200: 59-68 us against 28.4; 2000 x 1000 f32:
// 291 against 308).
static void plan_fused_eval(Plan& P, int64_t n_obs, const Switches& sw)
{
    const std::vector<int32_t>& startE = P.ordE.start;
    const std::vector<int32_t>& otherE = P.ordE.other;
    int n_act = 0;
    for (int q = 0; q < P.n_e; ++q)
        n_act += startE[q + 1] > startE[q];
    P.fused_eval = sw.eval_fused && n_act > 0;
    if (!P.fused_eval)
        return;
    P.fused_n_e_act = n_act;
    P.fused_f_pad = round_up(P.n_f, 64);
    P.fused_chunks = P.fused_f_pad / 64;
    // eliminated poses per wave: about one wave per SIMD in flight (1024 SIMDs), at most 16
    P.fused_group = std::min(16, std::max(1, (int)(((int64_t)n_act * P.fused_chunks + 500) / 1000)));
    if (sw.fused_group > 0)
        P.fused_group = sw.fused_group;
    P.fused_groups = (n_act + P.fused_group - 1) / P.fused_group;
    std::vector<int32_t> pair((size_t)P.n_e * P.fused_f_pad, -1), e_list, part0((size_t)P.n_e, 0), ptask((size_t)P.n_e + 1, 0);
    int slot = 0;
    for (int q = 0; q < P.n_e; ++q) {
        ptask[(size_t)q] = slot;
        part0[(size_t)q] = slot;
        if (startE[q + 1] > startE[q]) {
            e_list.push_back(q);
            slot += P.fused_chunks;
        }
        // a pair observed twice keeps its last observation here: such input is not supported by the dense
        // elimination either (one Z block per pair)
        for (int32_t d = startE[q]; d < startE[q + 1]; ++d)
            pair[(size_t)q * P.fused_f_pad + otherE[(size_t)d]] = d;
    }
    ptask[(size_t)P.n_e] = slot;
    // the lookup table cannot hold two observations of one pair: fall back to the two-pass kernel then
    int64_t n_in_table = 0;
    for (const int32_t v : pair)
        n_in_table += v >= 0;
    if (n_in_table != n_obs) {
        P.fused_eval = false;
        return;
    }
    P.fused_slots = slot;
    P.pair_obs.swap(pair);
    P.fused_e_list.swap(e_list);
    P.fused_e_part0.swap(part0);
    P.fused_pose_task.swap(ptask);
}

Plan make_plan(const vmm_ba_problem& p, const vmm_ba_create_options& co, bool elim_cams, bool multi, int world,
               bool points, const Switches& sw)
{
    Plan P;
    P.n_e = elim_cams ? p.n_cams : p.n_tags;
    P.n_f = elim_cams ? p.n_tags : p.n_cams;
    const int n_e = P.n_e, n_f = P.n_f;
    const int64_t n_obs = p.n_obs;

    // observation orders
    const int32_t* own_e = elim_cams ? p.obs_cam : p.obs_tag;
    const int32_t* own_f = elim_cams ? p.obs_tag : p.obs_cam;
    P.ordE = plan_order(n_e, own_e, own_f, p.obs_px, n_obs);
    P.ordF = plan_order(n_f, own_f, own_e, p.obs_px, n_obs);
    const std::vector<int32_t>& startE = P.ordE.start;
    const std::vector<int32_t>& otherE = P.ordE.other;
    const std::vector<int32_t>& callerE = P.ordE.caller;
    const std::vector<int32_t>& startF = P.ordF.start;
    const std::vector<int32_t>& callerF = P.ordF.caller;

    plan_fused_eval(P, n_obs, sw);

    // elimination / reduced system geometry
    P.n_red = 6 * n_f;
    P.n_pad = round_up(P.n_red, kNB);
    P.n_blk = P.n_pad / kNB;
    // >= n_pad + 64; the rank-k update reads whole 128-wide tiles.  The extra 32 doubles (256 B) make the row
    // stride an odd multiple of 256 B, so the 64 rows of a tile spread over the HBM channels instead of
    // hitting a few of them (a 48 KB stride at 2000 x 1000 does)
    P.ldz = round_up(P.n_pad + 1, kST) + 32;
    P.k_dim = 6 * n_e;
    P.k_pad = round_up(P.k_dim, kKT);
    // Reduced-system formation: dense Z + MFMA rank-k update, or compressed Z + the pair-list kernel.  Both are
    // priced per launch from the block structure (measured at 500 x 200, profiles/r03_sparse_*: the dense update + its
    // partial-tile sum take 118 us whatever the fill = 44 TFLOP/s; k_schur_pairs 16 us at 6-10 tags per image, 57 us at
    // 25 % and 116 us at 50 % visibility, priced as 18 us + 9 TFLOP/s of useful 6x6x6 block products);
    // VMM_BA_SCHUR=dense|sparse overrides.
    // World > 1: every decision that shapes the reduced system (its form is free per rank, its LAYOUT is not: the ranks'
    // systems are summed) is taken from the structure of ALL ranks' observations when the caller passes it
    // (vmm_ba_create_options.structure_obs_*), else from this rank's own -- and then the layout stays the natural one.
    // gStart / gOther: per eliminated pose the kept poses it sees (family-local indices), this rank's or everybody's.
    std::vector<int32_t> gStartV, gOtherV;
    const bool have_structure = co.n_structure_obs > 0 && co.structure_obs_cam && co.structure_obs_tag;
    if (multi && have_structure) {
        gStartV.assign((size_t)n_e + 1, 0);
        for (int64_t d = 0; d < co.n_structure_obs; ++d) {
            const int32_t c = co.structure_obs_cam[d], t = co.structure_obs_tag[d];
            if (c < 0 || c >= p.n_cams || t < 0 || t >= p.n_tags) {
                P.error = "structure_obs index out of range";
                return P;
            }
            if (points) {
                P.error = "structure_obs is not supported with point landmarks";
                return P;
            }
            gStartV[(size_t)(elim_cams ? c : t) + 1]++;
        }
        for (int q = 0; q < n_e; ++q)
            gStartV[(size_t)q + 1] += gStartV[(size_t)q];
        gOtherV.resize((size_t)co.n_structure_obs);
        std::vector<int32_t> fillg(gStartV.begin(), gStartV.end() - 1);
        for (int64_t d = 0; d < co.n_structure_obs; ++d) {
            const int32_t c = co.structure_obs_cam[d], t = co.structure_obs_tag[d];
            gOtherV[(size_t)fillg[(size_t)(elim_cams ? c : t)]++] = elim_cams ? t : c;
        }
    }
    const bool global_lists = !gStartV.empty();
    const std::vector<int32_t>& gStart = global_lists ? gStartV : startE;
    const std::vector<int32_t>& gOther = global_lists ? gOtherV : otherE;
    // one layout for all ranks: this rank alone (also the one-rank test hook), or everybody's structure in hand
    const bool layout_free = !multi || world == 1 || global_lists;
    {
        double pairs = 0.0;   // 6x6 block products of the lower triangle: sum over e of deg (deg + 1) / 2
        P.co_terms = 0.0;
        for (int q = 0; q < n_e; ++q) {
            const double deg = (double)(gStart[q + 1] - gStart[q]);
            pairs += 0.5 * deg * (deg + 1.0);
            P.co_terms += deg * deg;   // entries the host's adjacency lists of the kept family would hold before merging
        }
        const double dense_flops = (double)(P.n_pad + 1) * (P.n_pad + 2) * P.k_dim;
        const double n_obs_model = global_lists ? (double)co.n_structure_obs : (double)n_obs;
        const double sparse_flops = 432.0 * pairs + 72.0 * n_obs_model;
        const double dense_us = dense_flops / 44e6 + 12.0, sparse_us = sparse_flops / 9e6 + 18.0;
        // The plan of the block-sparse form lists every term: one (left, right) position pair per product plus the
        // right-hand-side term of every observation -- known from the degrees alone, before anything is allocated.  16 bytes
        // per term on the host while it is built, 8 on the device: the automatic choice stays below 4e7 terms (0.64 GB
        // transient, 0.32 GB resident; 2000 x 1000 at 25 % visibility would be 6e7), a forced one below the 2^31 the
        // 32-bit positions can address.
        const double plan_terms = pairs + n_obs_model;
        P.sparse_schur = n_obs_model > 0 && sparse_us < dense_us && plan_terms <= 4e7;
        if (sw.schur == 1)
            P.sparse_schur = false;
        else if (sw.schur == 2)
            P.sparse_schur = n_obs_model > 0;
        if (P.sparse_schur && plan_terms >= 2147483647.0) {
            P.error = "block-sparse elimination: more than 2^31 block products (set VMM_BA_SCHUR=dense)";
            return P;
        }
        P.schur_flops = P.sparse_schur ? sparse_flops : dense_flops;
    }
    std::vector<std::vector<int32_t>> tree_nbr;   // co-observation graph of the kept family (all ranks' when known)
    // Tree ordering of the kept family (VMM_BA_ORDER=nd; block-sparse path; world > 1: with the global structure): every node of the dissection tree
    // starts on a 64-row boundary of the reduced system (padding rows with a unit diagonal in between), so that whole
    // block columns of the factor belong to one node and the block columns of two parts of one level are independent.
    // (the host-side graph work is bounded: 5e7 list entries, and a natural order beyond the one-launch kernel's 48 block
    // columns cannot become a tree order within them)
    if (P.sparse_schur && layout_free && !sw.order_natural && n_f > 1 && P.n_blk >= 4 && P.co_terms <= 5e7) {
        std::vector<std::vector<int32_t>>& nbr = tree_nbr;
        nbr.assign((size_t)n_f, {});
        for (int q = 0; q < n_e; ++q)
            for (int32_t d1 = gStart[q]; d1 < gStart[q + 1]; ++d1)
                for (int32_t d2 = gStart[q]; d2 < gStart[q + 1]; ++d2)
                    if (d1 != d2)
                        nbr[(size_t)gOther[(size_t)d1]].push_back(gOther[(size_t)d2]);
        for (auto& v : nbr) {
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
        }
        std::vector<int32_t> all((size_t)n_f), stamp((size_t)n_f, 0);
        for (int fq = 0; fq < n_f; ++fq)
            all[(size_t)fq] = fq;
        int32_t stamp_next = 1;
        // tags per leaf: 42 = four 64-row blocks (21 and 10 measured slower on the close-up scene); VMM_BA_ND_LEAF
        std::vector<std::vector<int32_t>> nodes;
        nd_dissect(nbr, all, sw.nd_leaf, 12, stamp, stamp_next, nodes);
        std::vector<int32_t> rows((size_t)n_f, -1);
        int row = 0;
        for (const auto& nd : nodes) {
            row = round_up(row, kNB);
            for (const int32_t v : nd) {
                rows[(size_t)v] = row;
                row += 6;
            }
        }
        const int n_pad_nd = round_up(row, kNB);
        // Worth it?  The factorisation is a chain of dependent block columns (~11 us each): the longest chain under
        // the tree ordering (block structure after symbolic fill, nodes as dense blocks: an upper bound) against the
        // n_blk of the natural order.  Taken when it is at most 0.7 of it (VMM_BA_ORDER=nd: always).
        // (the block structure is kept as kDfMaskWords 64-bit words per block row, the panel order in bytes: at most 255
        // block columns; only the non-zero blocks of the factor get a workgroup, so the one-launch kernel takes the
        // system whatever its order -- counted below)
        const int nb = n_pad_nd / kNB;
        bool take = nodes.size() > 2 && nb <= kDfMaxBlk - 1;
        if (take) {
            const std::vector<BlkMask> nzr = symbolic_factor(nb, rows, nbr);
            int n_wg = nb;
            for (int i = 0; i < nb; ++i)
                for (int k = 0; k < i; ++k)
                    n_wg += nzr[(size_t)i].test(k) ? 1 : 0;
            n_wg += nb;   // the right-hand side row's block of every column
            int path_max = 1;
            const double t_tree = model_tree_factorisation(nb, nzr, nullptr, &path_max, sw.tree_model_r3);
            // natural order: the one-launch kernel up to 48 block columns (~9.8 us each), one launch per column beyond
            // (~32 us each at 94 columns)
            const double t_nat = P.n_blk <= 48 ? 9.8 * P.n_blk : 32.0 * P.n_blk;
            take = n_wg <= sw.tree_max_wg && (sw.order_nd || (path_max * 10 <= P.n_blk * 7 && t_tree <= 0.9 * t_nat));
            if (sw.debug)
                fprintf(stderr, "[vmm_ba debug] tree ordering candidate: longest chain %d of %d block columns against %d in "
                                "natural order, %d workgroups, modelled %.0f against %.0f us -> %s\n", path_max, nb, P.n_blk,
                        n_wg, t_tree, t_nat, take ? "taken" : "not taken");
        }
        if (take) {
            P.h_row_of = rows;
            int r2 = 0;
            for (const auto& nd : nodes) {
                r2 = round_up(r2, kNB);
                P.nd_node_first_blk.push_back(r2 / kNB);
                r2 += 6 * (int)nd.size();
            }
            P.n_pad = n_pad_nd;
            P.n_blk = P.n_pad / kNB;
            P.ldz = round_up(P.n_pad + 1, kST) + 32;
            if (sw.debug) {
                fprintf(stderr, "[vmm_ba debug] tree ordering: %zu nodes, %d rows (%d blocks) for %d kept poses; node sizes:",
                        nodes.size(), P.n_pad, P.n_blk, n_f);
                for (const auto& nd : nodes)
                    fprintf(stderr, " %zu", nd.size());
                fprintf(stderr, "\n");
            }
        }
    }
    if (!P.sparse_schur)
        return P;

    // F-order <-> E-order positions of an observation
    std::vector<int32_t> posE((size_t)n_obs), row_pos((size_t)n_obs);
    P.f2e.assign((size_t)n_obs, 0);
    for (int64_t d = 0; d < n_obs; ++d)
        posE[(size_t)callerE[(size_t)d]] = (int32_t)d;
    for (int fq = 0; fq < n_f; ++fq)
        for (int32_t d = startF[fq]; d < startF[fq + 1]; ++d) {
            P.f2e[(size_t)d] = posE[(size_t)callerF[(size_t)d]];
            row_pos[(size_t)P.f2e[(size_t)d]] = d - startF[fq];   // position of the observation in its kept pose's row
        }
    // The symbolic structure of S -= Z^T Z, once per problem (the counterpart of the symbolic phase of the sparse
    // Cholesky behind ceres::Solve): row f owns the pairs (f, f' = 0..f) and, last, its right-hand side entry.
    // A term of pair (f, f') = two observations (e, f), (e, f') of one eliminated pose; terms are listed in e
    // order (that is the summation order), the left block by its position in f's row (the kernel stages the
    // row's blocks in LDS), the right block by its E-order index.
    // Two forms of the pair list.  Implicit (every pair of the lower triangle, the empty ones written as zeros:
    // pair j of row f is f' = j): visibility-type scenes, where nearly every pair exists.  Explicit (only the pairs
    // that share an eliminated pose, their column in `pair_col`; S is zero-filled by a kernel of its own first):
    // scenes where an image sees a handful of tags -- at 6-10 tags per image 3.4 k of the 20.1 k pairs exist.  The
    // explicit form also carries the position of every kept pose in the reduced system (`row_of`), which need not
    // be 6 f (tree orderings of the kept family).
    const bool tree = !P.h_row_of.empty();
    std::vector<int32_t> rank_of((size_t)n_f);                  // order of the kept poses in the reduced system
    for (int fq = 0; fq < n_f; ++fq)
        rank_of[(size_t)fq] = tree ? P.h_row_of[(size_t)fq] : fq;
    std::vector<std::vector<int32_t>> partners;                    // explicit form: f' of every pair of row f
    {
        double co_pairs = 0.0;   // co-observed pairs incl. the diagonal, counted once
        std::vector<std::vector<int32_t>> adj((size_t)n_f);
        const bool list_pairs = tree || P.co_terms <= 5e7;   // else: the implicit form
        for (int q = 0; q < n_e && list_pairs; ++q)
            for (int32_t d1 = startE[q]; d1 < startE[q + 1]; ++d1)
                for (int32_t d2 = startE[q]; d2 < startE[q + 1]; ++d2) {
                    const int f1 = otherE[(size_t)d1], f2 = otherE[(size_t)d2];
                    if (rank_of[(size_t)f2] < rank_of[(size_t)f1])
                        adj[(size_t)f1].push_back(f2);
                }
        for (int fq = 0; fq < n_f; ++fq) {
            std::vector<int32_t>& a = adj[(size_t)fq];
            std::sort(a.begin(), a.end(), [&](int32_t x, int32_t y) { return rank_of[(size_t)x] < rank_of[(size_t)y]; });
            a.erase(std::unique(a.begin(), a.end()), a.end());
            a.push_back(fq);   // the diagonal pair: always there (it carries the kept pose's own block)
            co_pairs += (double)a.size();
        }
        const double all = 0.5 * (double)n_f * (n_f + 1.0);
        P.explicit_pairs = tree || (list_pairs && co_pairs < 0.5 * all);
        if (sw.pairs >= 0)
            P.explicit_pairs = tree || (list_pairs && sw.pairs == 1);
        if (P.explicit_pairs)
            partners.swap(adj);
    }
    std::vector<int32_t>& pstart = P.pair_start;
    pstart.assign((size_t)n_f + 1, 0);
    for (int fq = 0; fq < n_f; ++fq)
        pstart[(size_t)fq + 1] = pstart[(size_t)fq] + (P.explicit_pairs ? (int32_t)partners[(size_t)fq].size() + 1 : fq + 2);
    const size_t n_pairs = (size_t)pstart[(size_t)n_f];
    if (P.explicit_pairs) {
        P.pair_col.assign(n_pairs, -1);
        for (int fq = 0; fq < n_f; ++fq)
            for (size_t k = 0; k < partners[(size_t)fq].size(); ++k)
                P.pair_col[(size_t)pstart[(size_t)fq] + k] = tree ? P.h_row_of[(size_t)partners[(size_t)fq][k]]
                                                                   : 6 * partners[(size_t)fq][k];
    }
    // (f1, f2) -> pair id or -1.  Explicit: binary search in row f1's partner list (sorted by rank).
    auto pair_id = [&](int f1, int f2) -> int64_t {
        if (!P.explicit_pairs)
            return f2 <= f1 ? (int64_t)pstart[(size_t)f1] + f2 : -1;
        if (rank_of[(size_t)f2] > rank_of[(size_t)f1])
            return -1;
        const std::vector<int32_t>& a = partners[(size_t)f1];
        const auto it = std::lower_bound(a.begin(), a.end(), f2,
                                         [&](int32_t x, int32_t y) { return rank_of[(size_t)x] < rank_of[(size_t)y]; });
        return (int64_t)pstart[(size_t)f1] + (it - a.begin());
    };
    auto rhs_id = [&](int f1) -> int64_t { return (int64_t)pstart[(size_t)f1 + 1] - 1; };
    std::vector<int32_t>& tstart = P.pair_tstart;
    tstart.assign(n_pairs + 1, 0);
    for (int q = 0; q < n_e; ++q)
        for (int32_t d1 = startE[q]; d1 < startE[q + 1]; ++d1) {
            const int f1 = otherE[(size_t)d1];
            tstart[(size_t)rhs_id(f1) + 1]++;   // rhs pair of row f1
            for (int32_t d2 = startE[q]; d2 < startE[q + 1]; ++d2) {
                const int64_t id = pair_id(f1, otherE[(size_t)d2]);
                if (id >= 0)
                    tstart[(size_t)id + 1]++;
            }
        }
    for (size_t k = 0; k < n_pairs; ++k)
        tstart[k + 1] += tstart[k];
    const size_t n_terms = (size_t)tstart[n_pairs];
    if (n_terms >= ((size_t)1 << 31)) {
        P.error = "block-sparse elimination: more than 2^31 block products (set VMM_BA_SCHUR=dense)";
        return P;
    }
    std::vector<int32_t> ta(n_terms), tb(n_terms), fill(tstart.begin(), tstart.end() - 1);
    for (int q = 0; q < n_e; ++q)
        for (int32_t d1 = startE[q]; d1 < startE[q + 1]; ++d1) {
            const int f1 = otherE[(size_t)d1];
            {
                const int32_t k = fill[(size_t)rhs_id(f1)]++;
                ta[(size_t)k] = row_pos[(size_t)d1];
                tb[(size_t)k] = q;
            }
            for (int32_t d2 = startE[q]; d2 < startE[q + 1]; ++d2) {
                const int64_t id = pair_id(f1, otherE[(size_t)d2]);
                if (id < 0)
                    continue;
                const int32_t k = fill[(size_t)id]++;
                ta[(size_t)k] = row_pos[(size_t)d1];
                tb[(size_t)k] = d2;
            }
        }
    // the kernel walks a pair's terms pass by pass of 128 left blocks: terms must be ordered by left position.
    // They are listed in e order; a row's positions follow the caller's order, which need not be e order.
    for (size_t k = 0; k < n_pairs; ++k) {
        const int32_t t0 = tstart[k], t1 = tstart[k + 1];
        bool sorted = true;
        for (int32_t t = t0 + 1; t < t1 && sorted; ++t)
            sorted = ta[(size_t)t - 1] <= ta[(size_t)t];
        if (!sorted) {
            std::vector<std::pair<int32_t, int32_t>> tmp;
            for (int32_t t = t0; t < t1; ++t)
                tmp.emplace_back(ta[(size_t)t], tb[(size_t)t]);
            std::stable_sort(tmp.begin(), tmp.end(),
                             [](const std::pair<int32_t, int32_t>& x, const std::pair<int32_t, int32_t>& y) { return x.first < y.first; });
            for (int32_t t = t0; t < t1; ++t) {
                ta[(size_t)t] = tmp[(size_t)(t - t0)].first;
                tb[(size_t)t] = tmp[(size_t)(t - t0)].second;
            }
        }
    }
    P.pair_terms.assign(2 * std::max<size_t>(n_terms, 1), 0);
    for (size_t k = 0; k < n_terms; ++k) {
        P.pair_terms[2 * k] = ta[k];
        P.pair_terms[2 * k + 1] = tb[k];
    }
    // work items: up to kPairsPerItem consecutive pairs of one row; rows with many pairs first
    std::vector<int32_t> item_row, item_p0;
    std::vector<int32_t> rows_by_len((size_t)n_f);
    for (int fq = 0; fq < n_f; ++fq)
        rows_by_len[(size_t)fq] = n_f - 1 - fq;
    if (P.explicit_pairs)
        std::stable_sort(rows_by_len.begin(), rows_by_len.end(), [&](int32_t x, int32_t y) {
            return pstart[(size_t)x + 1] - pstart[(size_t)x] > pstart[(size_t)y + 1] - pstart[(size_t)y];
        });
    for (const int32_t fq : rows_by_len)
        for (int j0 = 0; j0 < pstart[(size_t)fq + 1] - pstart[(size_t)fq]; j0 += kPairsPerItem) {
            item_row.push_back(fq);
            item_p0.push_back(pstart[(size_t)fq] + j0);
        }
    P.n_row_items = (int)item_row.size();
    P.row_items = item_row;
    P.row_items.insert(P.row_items.end(), item_p0.begin(), item_p0.end());
    if (tree) {
        // Block structure of the factor under the tree ordering (symbolic_factor): from the co-observation graph the
        // ordering was made from -- ALL observations (an observation mask only removes entries), all ranks' with
        // world > 1 (the summed system has an entry wherever any rank has one).
        const int nb = P.n_blk;
        const std::vector<BlkMask> nzr = symbolic_factor(nb, P.h_row_of, tree_nbr);
        P.chol_nz.assign((size_t)(nb + 1) * kDfMaskWords, 0);
        for (int i = 0; i <= nb; ++i)
            for (int w = 0; w < kDfMaskWords; ++w)
                P.chol_nz[(size_t)i * kDfMaskWords + w] = nzr[(size_t)i].w[w];
        {
            // what this factorisation computes: per block column the diagonal block (d^3 / 3), a triangular solve per
            // non-zero block below it (d^3), a product per pair of them (2 d^3; d^3 on the diagonal), the right-hand
            // side row with them (2 d^2 per block), and the back-substitution (2 d^2 per block)
            const double d = (double)kNB;
            double fl = 0.0;
            for (int j2 = 0; j2 < nb; ++j2) {
                int nbl = 0;
                for (int r = j2 + 1; r < nb; ++r)
                    nbl += nzr[(size_t)r].test(j2) ? 1 : 0;
                fl += d * d * d / 3.0 + nbl * d * d * d + (double)nbl * nbl * d * d * d + 4.0 * (nbl + 1) * d * d;
            }
            P.chol_flops = fl;
        }
        // In which order does block column j take the panels it depends on?  In the order they are expected to be
        // finished, from the model of the kernel.
        P.chol_order.assign((size_t)nb * kDfMaxBlk, 0);
        int path_max = 0;
        const double t_model = model_tree_factorisation(nb, nzr, &P.chol_order, &path_max, sw.tree_model_r3);
        // The launch: one workgroup per non-zero block below the diagonal (the right-hand side row's last) and the
        // diagonal-only workgroup, panel-major -- a workgroup only ever waits for workgroups in front of it -- and one
        // slot of published slices per block that has a workgroup.
        P.df_slot.assign((size_t)nb * (nb + 1), -1);
        int32_t n_slots = 0;
        for (int j2 = 0; j2 < nb; ++j2) {
            for (int r = j2 + 1; r <= nb; ++r)
                if (r == nb || nzr[(size_t)r].test(j2)) {
                    P.df_wg.push_back(j2);
                    P.df_wg.push_back(r);
                    P.df_slot[(size_t)j2 * (nb + 1) + r] = n_slots++;
                }
            P.df_wg.push_back(j2);
            P.df_wg.push_back(j2);
        }
        P.n_df_wg = (int)(P.df_wg.size() / 2);
        P.df_tree_slots = (size_t)n_slots;
        if (sw.debug) {
            fprintf(stderr, "[vmm_ba debug] factor: longest chain %d of %d block columns, modelled %.0f us, %d workgroups, "
                            "%d of %d lower blocks\n", path_max, nb, t_model, P.n_df_wg, n_slots - nb + nb,
                    nb * (nb + 1) / 2);
            if (nb <= 64)
                for (int i = 0; i < nb; ++i) {
                    fprintf(stderr, "[vmm_ba debug]   %2d ", i);
                    for (int k = 0; k <= i; ++k)
                        fputc(nzr[(size_t)i].test(k) ? 'x' : '.', stderr);
                    fputc('\n', stderr);
                }
        }
    }
    if (P.explicit_pairs) {
        P.row_of.resize((size_t)n_f);
        for (int fq = 0; fq < n_f; ++fq)
            P.row_of[(size_t)fq] = tree ? P.h_row_of[(size_t)fq] : 6 * fq;
        if (multi && tree) {
            // world > 1 with a tree ordering: which kept pose a row of the reduced system belongs to (-1: padding), for the
            // kernel that adds the kept family's diagonal blocks behind the all-reduce (k_unpack_diag)
            P.pose_of_row.assign((size_t)P.n_pad, -1);
            for (int fq = 0; fq < n_f; ++fq)
                for (int k = 0; k < 6; ++k)
                    P.pose_of_row[(size_t)P.row_of[(size_t)fq] + k] = fq;
        }
    }
    return P;
}

} // namespace vmm
