// tests/lib_plan (TEST INFRASTRUCTURE ONLY): the pure pieces of the library path's host code
// (csrc/shs_lib_plan.hpp) checked on the CPU: build_rt_order, build_draw_table, plan_lib_pass,
// shadow_covers / shadow_union.  No HIP call, no libshs_gpu.so; exit status 0 = every check held.
#include <cstdio>
#include <random>
#include <set>

#include "../../leisure-software-renderer_amd/csrc/shs_lib_plan.hpp"

using namespace shs_plan;
using shs_dev::region_empty;

static int g_fail = 0, g_checks = 0;
#define CHECK(c)                                                                \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(c)) { ++g_fail; std::printf("%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); } \
    } while (0)

// ---- build_rt_order ----------------------------------------------------------------------------
static int g_xcd_cases = 0;   // st = 2 cases where all eight lists held something

static void rt_order_case(int tx, int ty, int rtiles_y, int rank, int count, const ShardRegion &reg, int st) {
    const std::vector<int32_t> out = build_rt_order(tx, ty, rtiles_y, rank, count, reg, st);
    std::vector<int32_t> want;   // (bin tile, row) ascending
    for (int t = 0; t < tx * ty; ++t) {
        const int bx = t % tx, by = t / tx;
        const bool owned = count <= 1 ? true : reg.on ? (bx >= reg.x0 && bx <= reg.x1 && by >= reg.y0 && by <= reg.y1) : t % count == rank;
        for (int r = 0; owned && r < RT_ROWS; ++r)
            if (by * RT_ROWS + r < rtiles_y) want.push_back((by * RT_ROWS + r) * tx + bx);
    }
    CHECK(out.size() == want.size());
    CHECK(std::multiset<int32_t>(out.begin(), out.end()) == std::multiset<int32_t>(want.begin(), want.end()));
    CHECK(std::set<int32_t>(out.begin(), out.end()).size() == out.size());
    if (st == 0) { CHECK(out == want); return; }
    const int nsx = (tx + st - 1) / st;
    auto list_of = [&](int32_t rt) {
        const int sx = (rt % tx) / st, sy = ((rt / tx) / RT_ROWS) / st;
        return ((sy * nsx + sx) + 3 * sy) & 7;
    };
    size_t len[8] = {};
    for (int32_t rt : want) ++len[list_of(rt)];
    const size_t shortest = *std::min_element(len, len + 8);
    if (shortest) ++g_xcd_cases;
    for (size_t j = 0; j < 8 * shortest && j < out.size(); ++j) CHECK(list_of(out[j]) == (int)(j % 8));
    // ... and throughout, round m takes one tile of every list that still has one, in list order
    size_t j = 0;
    for (size_t m = 0; j < out.size() && m < out.size(); ++m)
        for (int x = 0; x < 8; ++x)
            if (m < len[x] && j < out.size()) CHECK(list_of(out[j++]) == x);
    CHECK(j == out.size());
}

static void test_rt_order() {
    // (9 x 5 with st = 2 deals its supertiles over five of the eight lists; 17 x 2 fills all eight)
    const int grids[4][2] = {{1, 1}, {3, 2}, {9, 5}, {17, 2}};
    for (const auto &g : grids)
        for (int cut = 0; cut < 4; ++cut)   // the last bin row holds 4, 3, 2, 1 raster rows
            for (int st : {0, 2}) {
                const int tx = g[0], ty = g[1], rty = ty * RT_ROWS - cut;
                const ShardRegion none{0, 0, 0, 0, 0};
                rt_order_case(tx, ty, rty, 0, 1, none, st);
                for (int rank = 0; rank < 3; ++rank) rt_order_case(tx, ty, rty, rank, 3, none, st);
                rt_order_case(tx, ty, rty, 1, 2, ShardRegion{1, tx / 3, ty / 2, tx - 1, ty - 1}, st);
                rt_order_case(tx, ty, rty, 0, 2, ShardRegion{1, 0, 0, tx / 2, 0}, st);
                rt_order_case(tx, ty, rty, 1, 2, ShardRegion{1, 1, 0, 0, -1}, st);   // empty
            }
    CHECK(g_xcd_cases > 0);
}

// ---- build_draw_table --------------------------------------------------------------------------
static std::vector<LibDrawGPU> make_draws(const std::vector<int> &n_tris) {
    std::vector<LibDrawGPU> d(n_tris.size());
    int32_t base = 0;
    for (size_t i = 0; i < d.size(); ++i) {
        std::memset(&d[i], 0, sizeof d[i]);
        d[i].n_tris = n_tris[i];
        d[i].tri_base = base;
        d[i].program = SHS_PROGRAM_PBR_MR;
        d[i].n_verts = 1000 + (int32_t)i;   // (something to tell the records apart)
        base += n_tris[i];
    }
    return d;
}

static void draw_table_case(const std::vector<int> &n_tris) {
    const std::vector<LibDrawGPU> draws = make_draws(n_tris);
    const size_t nd = draws.size();
    const int total = (int)lib_pass_tris(draws.data(), nd);
    const int sb = std::max(1, (total + SETUP_BLOCK - 1) / SETUP_BLOCK);
    const std::vector<LibDrawGPU> table = build_draw_table(draws, sb);
    const size_t int_bytes = ((nd + 1) + (size_t)sb) * sizeof(int32_t);
    CHECK(table.size() == nd + (int_bytes + sizeof(LibDrawGPU) - 1) / sizeof(LibDrawGPU));   // whole records
    CHECK((table.size() - nd) * sizeof(LibDrawGPU) >= int_bytes);
    CHECK(std::memcmp(table.data(), draws.data(), nd * sizeof(LibDrawGPU)) == 0);
    const int32_t *dbase = reinterpret_cast<const int32_t *>(table.data() + nd), *bdraw = dbase + nd + 1;
    for (size_t i = 0; i < nd; ++i) CHECK(dbase[i] == draws[i].tri_base);
    CHECK(dbase[nd] == total);
    for (int b = 0; b < sb; ++b) {
        int holder = -1;   // brute force: the draw holding triangle 256 b
        for (size_t i = 0; i < nd; ++i)
            if (draws[i].tri_base <= b * SETUP_BLOCK && b * SETUP_BLOCK < draws[i].tri_base + draws[i].n_tris) holder = (int)i;
        CHECK(holder >= 0 && bdraw[b] == holder);
    }
}

static void test_draw_table() {
    draw_table_case({1});
    draw_table_case({255, 1, 600});
    draw_table_case({255, 0, 600});
    draw_table_case({256, 0, 300});   // the empty draw starts on a block boundary
}

// ---- plan_lib_pass -----------------------------------------------------------------------------
namespace {
struct Pass {
    LibFrameParams desc;
    std::vector<LibDrawGPU> draws;
    shs_tonemap_desc tm;
    LibPassInputs in;
    Pass(int n_tris = 1000, bool shadow = false) : draws(make_draws({n_tris})) {
        std::memset(&desc, 0, sizeof desc);
        std::memset(&tm, 0, sizeof tm);
        desc.W = 96; desc.H = 64; desc.count = 1;
        in.shadow = shadow;
        in.extra_cap = 4096;
        in.n_owned_rt = 24;
    }
    // plans the pass and checks that every optional buffer's count is 0 exactly when its enabling field is off
    LibPassPlan plan() {
        in.desc = &desc;
        in.draws = draws.data();
        in.n_draws = draws.size();
        const LibPassPlan p = plan_lib_pass(in);
        const bool cam = !in.shadow;
        CHECK((p.n_shade != 0) == cam && (p.n_xbase != 0) == cam && (p.n_dynq != 0) == cam);
        CHECK(!cam || (p.n_shade == p.n_slots && p.n_xbase == (size_t)std::max(p.n_tris, 1)));
        CHECK((p.n_s2s != 0) == ((p.fp.flags & shs_dev::LF_PERM) != 0));
        CHECK((p.n_uvw != 0) == (cam && p.textured) && (!p.n_uvw || p.n_uvw == 2 * p.n_slots));
        CHECK((p.n_items != 0) == (p.fp.part != 0) && (p.n_pkeys != 0) == (p.fp.part != 0) && (p.n_pcount != 0) == (p.fp.part != 0));
        CHECK((p.fp.split_cap != 0) == (p.fp.part != 0));
        CHECK((p.n_hsq != 0) == (p.fp.hsort != 0) && (!p.n_hsq || p.n_hsq == (size_t)p.n_tiles));
        CHECK((p.n_blkrect != 0) == (cam && p.fp.count > 1 && p.fp.reg.on) && (!p.n_blkrect || p.n_blkrect == (size_t)p.setup_blocks));
        CHECK((p.n_tm_thr != 0) == (cam && in.tm));
        CHECK((p.n_tm_ldr != 0) == (cam && in.tm && (in.tm->flags & SHS_TONEMAP_LDR)));
        CHECK((p.n_tm_present != 0) == (cam && in.tm && (in.tm->flags & SHS_TONEMAP_PRESENT)));
        CHECK(p.timeline == (in.want_timeline && in.timeline_shadow == in.shadow));
        CHECK((p.n_stimeline != 0) == (cam && p.timeline));
        CHECK(p.side_stream == (cam && in.cam_after_shadow));
        CHECK(p.n_tile_count == 2 * (size_t)p.n_tiles && p.n_busy == (size_t)p.n_rt && p.n_bins == (size_t)p.n_tiles * in.bin_cap);
        CHECK(p.n_blk_stat == (size_t)p.setup_blocks && p.fp.setup_blocks == p.setup_blocks);
        return p;
    }
};
}  // namespace

static void test_plan_geometry_and_modes() {
    Pass a;   // 96 x 64: 3 x 2 bin tiles, 8 raster rows
    LibPassPlan p = a.plan();
    CHECK(p.tiles_x == 3 && p.tiles_y == 2 && p.n_tiles == 6 && p.rtiles_y == 8 && p.n_rt == 24);
    CHECK(p.n_tris == 1000 && p.setup_blocks == 4 && p.fp.n_draws == 1 && p.fp.n_owned_rt == 24);
    a.desc.H = 57;   // the same bin rows, another raster row count: a new (geom_key, rtiles_y) pair
    const LibPassPlan q = a.plan();
    CHECK(q.geom_key == p.geom_key && q.rtiles_y == 8 && q.tiles_y == 2);
    a.desc.H = 56;
    CHECK(a.plan().rtiles_y == 7 && a.plan().geom_key == p.geom_key);
    a.desc.W = 97;
    CHECK(a.plan().geom_key != p.geom_key);
    // scan / bins
    CHECK(Pass(SCAN_MAX_PRIMS).plan().fp.scan_mode == 1u);
    CHECK(Pass(SCAN_MAX_PRIMS + 1).plan().fp.scan_mode == 0u);
    Pass e(0);
    e.draws.clear();
    p = e.plan();
    CHECK(p.n_tris == 0 && p.setup_blocks == 1 && p.n_slots == 1 + (size_t)e.in.extra_cap && p.fp.scan_mode == 1u);
    // parity
    a.in.frame_index = 7;
    CHECK(a.plan().fp.parity == 1u);
}

static void test_plan_shallow() {
    for (bool shadow : {false, true}) {
        Pass s(200, shadow);   // scan mode: the fullest list is n_tris + st_extra (camera only)
        s.in.st_checked = true;
        s.in.st_maxbin = 9999;   // (not read in scan mode)
        s.in.st_extra = SHALLOW_MAX - 200;
        CHECK(s.plan().shallow);
        s.in.st_extra = SHALLOW_MAX - 200 + 1;
        CHECK(s.plan().shallow == shadow);
        s.in.st_checked = false;   // never before the first check
        s.in.st_extra = 0;
        CHECK(!s.plan().shallow);
        Pass b(1000, shadow);   // bins: the previous pass's fullest bin
        b.in.st_checked = true;
        b.in.st_maxbin = SHALLOW_MAX;
        CHECK(b.plan().shallow);
        b.in.exp.force_deep = 1;   // the experiment's switch: camera passes only
        CHECK(b.plan().shallow == shadow);
        b.in.exp.force_deep = 0;
        b.in.st_maxbin = SHALLOW_MAX + 1;
        CHECK(!b.plan().shallow);
        b.in.st_checked = false;
        b.in.st_maxbin = 0;
        CHECK(!b.plan().shallow);
    }
}

static void test_plan_hsort() {
    auto base = [] {   // camera, bins, no parts, deep, the previous pass had a long list
        Pass p(1000);
        p.in.st_checked = true;
        p.in.st_maxbin = shs_dev::LIB_HSORT_MIN + 1;
        return p;
    };
    CHECK(base().plan().fp.hsort == 1u && base().plan().fp.hsort_min == shs_dev::LIB_HSORT_MIN);
    { Pass p = base(); p.in.shadow = true; CHECK(p.plan().fp.hsort == 0u); }
    { Pass p = base(); p.draws = make_draws({SCAN_MAX_PRIMS}); CHECK(p.plan().fp.hsort == 0u); }
    { Pass p = base(); p.in.lib_part = 128; CHECK(p.plan().fp.hsort == 0u); }
    { Pass p = base(); p.in.st_maxbin = SHALLOW_MAX; CHECK(p.plan().shallow && p.plan().fp.hsort == 0u); }
    { Pass p = base(); p.in.st_maxbin = shs_dev::LIB_HSORT_MIN; CHECK(!p.plan().shallow && p.plan().fp.hsort == 0u); }
    { Pass p = base(); p.in.st_checked = false; p.in.st_maxbin = 0; CHECK(p.plan().fp.hsort == 1u); }   // before the first check
}

static void test_plan_parts() {
    auto part_of = [](bool shadow, int n_tris, int64_t lib_part, int count) {
        Pass p(n_tris, shadow);
        p.in.lib_part = lib_part;
        p.desc.count = count;
        return p.plan().fp.part;
    };
    CHECK(part_of(false, 1000, 128, 1) == 128u && part_of(false, 1000, 128, 4) == 128u);
    CHECK(part_of(true, 1000, 128, 1) == 0u && part_of(true, 1000, -1, 4) == 0u);
    CHECK(part_of(false, SCAN_MAX_PRIMS, 128, 1) == 0u && part_of(false, SCAN_MAX_PRIMS, -1, 4) == 0u);
    CHECK(part_of(false, 1000, -1, 4) == AUTO_PART && part_of(false, 1000, -1, 2) == AUTO_PART);
    CHECK(part_of(false, 1000, -1, 1) == 0u && part_of(false, 1000, 0, 4) == 0u);
    for (int owned : {0, 1, 100, SPLIT_CAP_MAX, SPLIT_CAP_MAX + 1, 20000}) {
        Pass p;
        p.in.lib_part = 128;
        p.in.n_owned_rt = owned;
        const LibPassPlan q = p.plan();
        CHECK(q.fp.split_cap == (uint32_t)std::min(std::max(owned, 1), SPLIT_CAP_MAX));
        CHECK(q.n_items == (size_t)std::max(owned, 1) * shs_dev::LIB_MAXK && q.n_pcount == q.fp.split_cap);
        CHECK(q.n_pkeys == (size_t)q.fp.split_cap * shs_dev::LIB_RTH_PX);
        CHECK(q.fp.dyn_cap == (uint32_t)(((size_t)std::max(owned, 1) * (1 + shs_dev::LIB_MAXK) + shs_dev::LIB_NQ - 1) / shs_dev::LIB_NQ + 1));
        CHECK(q.n_dynq == (size_t)2 * shs_dev::LIB_NQ * q.fp.dyn_cap);
    }
}

static void test_plan_listed() {
    auto base = [] {   // camera, bins, sharded, interleaved, SHS_OPT_SHARD_CULL on
        Pass p(1000);
        p.desc.count = 4;
        p.desc.rank = 1;
        p.in.shard_cull = true;
        return p;
    };
    CHECK(base().plan().listed);
    { Pass p = base(); p.in.shadow = true; CHECK(!p.plan().listed); }
    { Pass p = base(); p.draws = make_draws({SCAN_MAX_PRIMS}); CHECK(!p.plan().listed); }
    { Pass p = base(); p.desc.count = 1; p.desc.rank = 0; CHECK(!p.plan().listed); }
    { Pass p = base(); p.desc.reg = ShardRegion{1, 0, 0, 1, 1}; CHECK(!p.plan().listed && p.plan().n_blkrect == 4); }
    { Pass p = base(); p.in.shard_cull = false; CHECK(!p.plan().listed); }
}

static void test_plan_capacities_and_flags() {
    for (int n : {100, 40000}) {
        Pass cam(n), sh(n, true);
        cam.in.extra_cap = sh.in.extra_cap = 0;   // first use
        const uint32_t first = (uint32_t)std::max(EXTRA_CAP_MIN, n / 4);
        LibPassPlan p = cam.plan(), q = sh.plan();
        CHECK(p.extra_cap == first && p.fp.extra_cap == first && p.n_slots == (size_t)n + first);
        CHECK(q.extra_cap == first && q.fp.extra_cap == 0u && q.n_slots == (size_t)n);   // a shadow pass has no extras
        cam.in.extra_cap = 5000;
        CHECK(cam.plan().extra_cap == 5000u && cam.plan().n_slots == (size_t)n + 5000);
    }
    Pass a;
    a.in.bin_cap = 512; a.in.spill_cap = 70000;
    CHECK(a.plan().fp.bin_cap == 512u && a.plan().fp.spill_cap == 70000u);
    a.in.spill_cap = (size_t)1 << 33;
    CHECK(a.plan().fp.spill_cap == 0xffffffffu);
    CHECK(a.plan().fp.static_div == 2 && a.plan().fp.heavy_min == 2048u && Pass(1000, true).plan().fp.heavy_min == 0u);
    // LF_PERM: only a camera pass with a permuted draw
    static const uint32_t some_order = 0;
    for (bool shadow : {false, true})
        for (bool perm : {false, true})
            for (uint32_t stale : {0u, (uint32_t)shs_dev::LF_PERM}) {
                Pass p(1000, shadow);
                p.draws = make_draws({300, 700});
                if (perm) p.draws[1].orig = &some_order;
                p.desc.flags = shs_dev::LF_DEPTH | stale;
                const LibPassPlan q = p.plan();
                CHECK(q.permuted == perm && ((q.fp.flags & shs_dev::LF_PERM) != 0) == (perm && !shadow));
                CHECK((q.fp.flags & ~shs_dev::LF_PERM) == shs_dev::LF_DEPTH);
            }
    Pass t;
    t.draws[0].tex = &some_order;
    CHECK(t.plan().textured && t.plan().n_uvw != 0);
    t.in.shadow = true;
    CHECK(t.plan().n_uvw == 0);
    // the fused tonemap
    Pass f;
    f.tm.flags = SHS_TONEMAP_LDR;
    f.tm.gamma = 0.0f; f.tm.exposure = 0.0f;
    f.in.tm = &f.tm;
    LibPassPlan p = f.plan();
    CHECK(p.n_tm_ldr == (size_t)96 * 64 && p.n_tm_present == 0 && p.tm_gamma == 0.001f && p.fp.tm_exposure == 0.0001f);
    CHECK(p.fp.tm_inv_gamma == 1.0f / 0.001f);
    f.tm.flags = SHS_TONEMAP_LDR | SHS_TONEMAP_PRESENT;
    f.tm.gamma = 2.2f; f.tm.exposure = 1.5f;
    p = f.plan();
    CHECK(p.n_tm_present == (size_t)96 * 64 && p.tm_gamma == 2.2f && p.fp.tm_exposure == 1.5f && p.fp.tm_inv_gamma == 1.0f / 2.2f);
    // timelines, the side stream
    for (bool shadow : {false, true})
        for (bool want : {false, true})
            for (bool tl_shadow : {false, true}) {
                Pass q(1000, shadow);
                q.in.want_timeline = want; q.in.timeline_shadow = tl_shadow; q.in.cam_after_shadow = want;
                q.plan();
            }
}

static void test_plan_resolve_variant() {
    auto variant = [](const std::vector<int> &programs, int count, int sky_model) {
        Pass p;
        p.draws = make_draws(std::vector<int>(programs.size(), 10));
        for (size_t i = 0; i < programs.size(); ++i) p.draws[i].program = programs[i];
        p.desc.count = count;
        p.desc.sky.model = sky_model;
        return p.plan();
    };
    const int PBR = SHS_PROGRAM_PBR_MR, FP = SHS_PROGRAM_FORWARD_PLUS, TY = SHS_PROGRAM_FORWARD_PLUS_TYPED;
    CHECK(variant({PBR, PBR}, 1, 0).prog == PBR && variant({FP, FP, FP}, 1, 0).prog == FP);
    CHECK(variant({PBR, FP}, 1, 0).prog == -1 && variant({SHS_PROGRAM_BLINN_PHONG}, 1, 0).prog == -1);
    CHECK(variant({PBR, TY}, 1, 0).prog == TY && variant({TY}, 1, 0).prog == TY && variant({FP, TY, PBR}, 1, 0).prog == TY);
    CHECK(variant({}, 1, 0).prog == -1);
    LibPassPlan p = variant({PBR}, 1, shs_dev::SKY_NONE);
    CHECK(p.wide && !p.sky);
    p = variant({PBR}, 2, shs_dev::SKY_CUBEMAP);
    CHECK(!p.wide && p.sky);
    CHECK(variant({PBR}, 1, shs_dev::SKY_PROCEDURAL).sky);
    std::set<int> slots;   // every build has its own slot of the resident-count table
    for (int prog : {FP, PBR, -1, TY})
        for (bool wide : {false, true})
            for (bool sky : {false, true}) {
                const int v = resolve_variant(prog, wide, sky);
                CHECK(v >= 0 && v < RESOLVE_VARIANTS);
                slots.insert(v);
            }
    CHECK((int)slots.size() == RESOLVE_VARIANTS);
}

// ---- shadow_covers / shadow_union --------------------------------------------------------------
static uint32_t sp(int x0, int x1) { return (uint32_t)x0 | ((uint32_t)x1 << 16); }

// brute force: the tiles of (region, span)
static std::set<int> tiles_of(const ShardRegion &g, const std::vector<uint32_t> &span) {
    std::set<int> s;
    for (int y = g.y0; y <= g.y1; ++y)
        for (int x = g.x0; x <= g.x1; ++x) {
            if (!span.empty() && ((size_t)y >= span.size() || x < (int)(span[(size_t)y] & 0xffffu) || x > (int)(span[(size_t)y] >> 16))) continue;
            s.insert(y * 64 + x);
        }
    return s;
}

static void test_shadow() {
    const std::vector<uint32_t> none;
    const ShardRegion empty{1, 0, 0, -1, -1}, big{1, 1, 1, 6, 5}, in{1, 2, 2, 4, 4};
    std::vector<uint32_t> us;
    CHECK(shadow_covers(big, none, empty, none) && shadow_covers(empty, none, empty, none));   // need is empty
    CHECK(!shadow_covers(empty, none, in, none));                                              // have is empty
    ShardRegion u = shadow_union(empty, none, in, {1u, 1u, sp(2, 3), sp(2, 4), sp(3, 4)}, us);
    CHECK(u.x0 == in.x0 && u.y1 == in.y1 && us.size() == 5 && us[2] == sp(2, 3));
    CHECK(shadow_covers(big, none, in, none) && !shadow_covers(in, none, big, none));          // need inside have
    const std::vector<uint32_t> hs = {1u, sp(1, 6), sp(2, 6), sp(1, 3), sp(2, 4), sp(1, 6)};
    CHECK(shadow_covers(big, hs, in, {1u, 1u, sp(2, 4), sp(2, 3), sp(2, 4)}));                 // ... with spans
    CHECK(!shadow_covers(big, hs, in, none));                                                  // row 3 has only columns 1..3
    CHECK(!shadow_covers(big, hs, in, {1u, 1u, sp(2, 4), sp(2, 4), sp(2, 4)}));
    CHECK(shadow_covers(big, hs, in, {1u, 1u, sp(2, 4), 1u, sp(2, 4)}));                       // a row whose needed span is empty
    CHECK(shadow_covers(big, hs, in, {1u, 1u, sp(2, 4), sp(5, 6), sp(2, 4)}));                 // ... empty inside the rectangle
    CHECK(!shadow_covers(big, hs, in, {1u, 1u, sp(2, 4)}));                                    // span vectors of different lengths:
    CHECK(!shadow_covers(big, {1u, sp(1, 6), sp(1, 6)}, in, none));                            // rows past either end are not known
    u = shadow_union(big, hs, in, {1u, 1u, sp(2, 4)}, us);
    CHECK(us.empty() && u.x0 == 1 && u.y0 == 1 && u.x1 == 6 && u.y1 == 5);                     // ... and unite to the rectangle
    u = shadow_union(big, none, in, {1u, 1u, sp(2, 4), sp(2, 4), sp(2, 4), 1u}, us);
    CHECK(us.empty());

    std::mt19937 rng(20240611);
    auto rnd = [&](int n) { return (int)(rng() % (uint32_t)n); };
    auto region = [&] {
        if (rnd(8) == 0) return ShardRegion{1, 1, 0, 0, -1};
        const int x0 = rnd(8), y0 = rnd(8);
        return ShardRegion{1, x0, y0, x0 + rnd(8 - x0), y0 + rnd(8 - y0)};
    };
    auto spans = [&](const ShardRegion &g) {
        std::vector<uint32_t> s;
        if (rnd(3) == 0 || region_empty(g)) return s;
        s.assign(8, 1u);
        for (int y = g.y0; y <= g.y1; ++y) {
            const int a = g.x0 + rnd(g.x1 - g.x0 + 1);
            s[(size_t)y] = rnd(5) == 0 ? 1u : sp(a, a + rnd(g.x1 - a + 1));
        }
        return s;
    };
    int n_cov = 0, n_not = 0;
    for (int it = 0; it < 600; ++it) {
        const ShardRegion have = region(), need = region();
        const std::vector<uint32_t> hsp = spans(have), nsp = spans(need);
        const std::set<int> th = tiles_of(have, hsp), tn = tiles_of(need, nsp);
        const bool cov = shadow_covers(have, hsp, need, nsp);
        if (cov) CHECK(std::includes(th.begin(), th.end(), tn.begin(), tn.end()));   // (it may say no where tiles would do)
        u = shadow_union(have, hsp, need, nsp, us);
        CHECK(shadow_covers(u, us, have, hsp) && shadow_covers(u, us, need, nsp));
        const bool comparable = !region_empty(have) && !hsp.empty() && hsp.size() == nsp.size();
        if (cov && !region_empty(need) && comparable) {   // nothing new: the union is what was rendered
            CHECK(u.x0 == have.x0 && u.y0 == have.y0 && u.x1 == have.x1 && u.y1 == have.y1);
            CHECK(tiles_of(u, us) == th);
        }
        (cov ? n_cov : n_not)++;
    }
    CHECK(n_cov > 50 && n_not > 50);
}

int main() {
    test_rt_order();
    test_draw_table();
    test_plan_geometry_and_modes();
    test_plan_shallow();
    test_plan_hsort();
    test_plan_parts();
    test_plan_listed();
    test_plan_capacities_and_flags();
    test_plan_resolve_variant();
    test_shadow();
    std::printf("lib_plan: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
