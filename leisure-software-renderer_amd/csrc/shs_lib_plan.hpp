// shs_lib_plan.hpp -- what a library pass decides before anything is allocated or launched, as pure
// functions of the pass description, the previous pass's statistics and the context's options: no HIP
// call, no context, no environment, no statics (tests/lib_plan compiles this header with plain g++).
// shs_abi_lib.cpp sizes, binds and launches what plan_lib_pass returns.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/shs_gpu.h"
#include "shs_lib_device.hpp"

#pragma GCC visibility push(hidden)
namespace shs_plan {

using shs_dev::LibDrawGPU;
using shs_dev::LibFrameParams;
using shs_dev::ShardRegion;

constexpr int BIN_TILE = 32;                 // shs_dev::TILE (shs_device.hpp is device code; asserted in shs_abi_lib.cpp)
constexpr int RT_ROWS = BIN_TILE / 8;        // raster rows per bin tile
constexpr int SETUP_BLOCK = 256;             // triangles per setup block
constexpr int64_t MAX_PASS_TRIS = 1 << 27;
// Smaller passes scan every primitive's box per busy tile (no bins); above this the per-tile bins win
// even for ~1.5K primitives (C5: raster 0.51 -> 0.44 ms, the gather was a 1.5K-box scan per tile).
constexpr int SCAN_MAX_PRIMS = 512;
constexpr uint32_t SHALLOW_MAX = 256;        // the shallow raster's candidate round
constexpr uint32_t AUTO_PART = 512;          // SHS_OPT_LIB_PART -1 on a sharded rank
constexpr int SPLIT_CAP_MAX = 8192;
constexpr int EXTRA_CAP_MIN = 4096;

// Timing-experiment overrides (the experiments build fills them from the environment; the product
// build leaves the defaults).
struct LibPlanExp {
    int xcd_st = 2;                  // SHS_LIB_XCD_ST: supertile edge in bin tiles (0 = plain order)
    long scan_max = SCAN_MAX_PRIMS;  // SHS_LIB_SCAN_MAX: the scan / bin threshold
    uint32_t exp_flags = 0;          // SHS_LIB_EXP: parts of the setup skipped
    int force_deep = 0;              // SHS_LIB_DEEP=1: the deep raster for every camera pass
    int static_div = 2;              // SHS_LIB_STATIC_DIV: static share of the raster items
    int heavy = 2048;                // SHS_LIB_HEAVY: heavy tiles (bin list entries; 0 = none)
};

struct LibPassInputs {
    bool shadow = false;                       // PassShadowMap's depth pass, else the camera pass
    const LibFrameParams *desc = nullptr;      // the pass as recorded: W, H, rank / count / reg, flags, sky, ...
    const LibDrawGPU *draws = nullptr;         // read: n_tris, tri_base, program, orig, tex
    size_t n_draws = 0;
    const shs_tonemap_desc *tm = nullptr;      // the fused tonemap, or null
    // the workspace's history (check_pass)
    bool st_checked = false;
    uint64_t st_maxbin = 0, st_extra = 0;
    uint32_t bin_cap = 256, extra_cap = 0, frame_index = 0;
    size_t spill_cap = 0;
    // the context's options
    int64_t lib_part = 0;
    bool shard_cull = false, cam_after_shadow = false, want_timeline = false, timeline_shadow = false;
    int n_owned_rt = 0;                        // the raster tile order's length (order cache)
    LibPlanExp exp;
};

struct LibPassPlan {
    int tiles_x, tiles_y, n_tiles, rtiles_y, n_rt;
    int n_tris, setup_blocks;
    size_t n_slots;                  // max(n_tris, 1) primaries + (camera pass) extra_cap
    uint32_t extra_cap;              // the workspace's (first use: max(4096, n_tris / 4)); fp.extra_cap is 0 for a shadow pass
    bool side_stream;                // setup and raster on the side stream (cam_after_shadow, camera pass)
    bool shallow, listed, permuted, textured;
    int prog;                        // k_lib_resolve's specialisation: the one program of every draw, or -1
    bool wide, sky;
    uint64_t geom_key;               // with rtiles_y: a change zeroes the per-tile state
    float tm_gamma;                  // fused tonemap: the clamped gamma of its thresholds
    // element counts of the optional buffers (0: not needed, the pointer stays null)
    size_t n_shade, n_xbase, n_s2s, n_uvw, n_items, n_pkeys, n_pcount, n_dynq, n_hsq, n_blkrect, n_tm_thr, n_tm_ldr,
        n_tm_present, n_stimeline;
    bool timeline;                   // the raster's timeline (LTL_STRIDE per workgroup of the caller's raster grid)
    // ... and of the ones every pass has
    size_t n_tile_count, n_busy, n_bins, n_blk_stat;
    LibFrameParams fp;               // complete but for raster_grid (the caller's occupancy query)
};

inline int64_t lib_pass_tris(const LibDrawGPU *draws, size_t n) {
    int64_t total = 0;
    for (size_t i = 0; i < n; ++i) total += draws[i].n_tris;
    return total;
}

// ctx->lib_resolve_resident's slot of a resolve build: (sky) x (Forward+, PBR, mixed, typed) x (wide).
constexpr int RESOLVE_VARIANTS = 2 * 4 * 2;
inline int resolve_variant(int prog, bool wide, bool sky) {
    const int p = prog == SHS_PROGRAM_FORWARD_PLUS ? 0 : prog == SHS_PROGRAM_PBR_MR ? 1 : prog == SHS_PROGRAM_FORWARD_PLUS_TYPED ? 3 : 2;
    return (sky ? 8 : 0) + p * 2 + (wide ? 1 : 0);
}

// What the draw list decides: permuted (a spatially ordered mesh: the resolve maps winners to slots through
// s2s), textured, and the resolve's program.
inline void plan_draws(const LibPassInputs &in, LibPassPlan &p) {
    p.prog = in.n_draws ? in.draws[0].program : -1;
    bool typed = false;
    for (size_t i = 0; i < in.n_draws; ++i) {
        const LibDrawGPU &d = in.draws[i];
        p.permuted = p.permuted || d.orig != nullptr;
        p.textured = p.textured || d.tex != nullptr;
        if (d.program != p.prog) p.prog = -1;
        typed = typed || d.program == SHS_PROGRAM_FORWARD_PLUS_TYPED;
    }
    if (p.prog != SHS_PROGRAM_FORWARD_PLUS && p.prog != SHS_PROGRAM_PBR_MR) p.prog = -1;
    if (typed) p.prog = SHS_PROGRAM_FORWARD_PLUS_TYPED;   // any typed Forward+ draw: the kernel with the light models
}

inline LibPassPlan plan_lib_pass(const LibPassInputs &in) {
    LibPassPlan p;
    std::memset(&p, 0, sizeof p);
    LibFrameParams &fp = p.fp;
    fp = *in.desc;
    const bool shadow = in.shadow;
    p.tiles_x = (fp.W + BIN_TILE - 1) / BIN_TILE;
    p.tiles_y = (fp.H + BIN_TILE - 1) / BIN_TILE;
    p.n_tiles = p.tiles_x * p.tiles_y;
    p.rtiles_y = (fp.H + 7) / 8;
    p.n_rt = p.tiles_x * p.rtiles_y;
    // rtiles_y too: a height change inside the same bin-tile rows changes the raster-tile rows
    p.geom_key = ((uint64_t)p.tiles_x << 48) ^ ((uint64_t)p.tiles_y << 32);
    const int n_tris = p.n_tris = (int)lib_pass_tris(in.draws, in.n_draws);
    p.extra_cap = in.extra_cap ? in.extra_cap : (uint32_t)std::max(EXTRA_CAP_MIN, n_tris / 4);
    p.n_slots = (size_t)std::max(n_tris, 1) + (shadow ? 0 : p.extra_cap);
    p.setup_blocks = std::max(1, (n_tris + SETUP_BLOCK - 1) / SETUP_BLOCK);
    p.side_stream = !shadow && in.cam_after_shadow;

    plan_draws(in, p);
    p.wide = fp.count <= 1;   // the whole frame's build (PBR: 5 waves) or a sharded rank's
    p.sky = fp.sky.model != shs_dev::SKY_NONE;   // the kernel's sky builds
    if (!shadow && p.permuted) fp.flags |= shs_dev::LF_PERM;
    else fp.flags &= ~shs_dev::LF_PERM;

    fp.tiles_x = p.tiles_x; fp.tiles_y = p.tiles_y; fp.rtiles_y = p.rtiles_y;
    fp.n_tris = n_tris;
    fp.n_draws = (int)in.n_draws;
    fp.bin_cap = in.bin_cap;
    fp.spill_cap = (uint32_t)std::min<size_t>(in.spill_cap, 0xffffffffu);
    fp.extra_cap = shadow ? 0u : p.extra_cap;
    fp.parity = in.frame_index & 1u;
    // scan mode (every busy tile tests every primitive's box) for small passes, per-tile bins above
    fp.scan_mode = n_tris <= in.exp.scan_max ? 1u : 0u;
    fp.setup_blocks = p.setup_blocks;
    fp.exp_flags = in.exp.exp_flags;
    fp.n_owned_rt = in.n_owned_rt;
    const size_t n_owned = (size_t)std::max(fp.n_owned_rt, 1);
    // Camera pass, tile-sharded: k_lib_plan splits the busy tiles whose bin list is longer than `part`
    // entries into parts rendered by several workgroups (SHS_OPT_LIB_PART: -1 auto = 512 when sharded,
    // 0 = off, else the part size for every camera pass).
    fp.part = 0u;
    if (!shadow && !fp.scan_mode) {
        if (in.lib_part > 0) fp.part = (uint32_t)in.lib_part;
        else if (in.lib_part < 0 && fp.count > 1) fp.part = AUTO_PART;
    }
    if (fp.part) {   // split tiles' key slots: KEY_EMPTY / 0 once, then reset by each tile's last part
        fp.split_cap = (uint32_t)std::min(std::max(fp.n_owned_rt, 1), SPLIT_CAP_MAX);
        p.n_items = n_owned * shs_dev::LIB_MAXK;
        p.n_pkeys = (size_t)fp.split_cap * shs_dev::LIB_RTH_PX;
        p.n_pcount = fp.split_cap;
    }
    // the shallow raster (256-candidate rounds, twice the workgroups per CU) when the previous frame's
    // fullest bin tile fit one such round (scan mode: every primitive is a candidate)
    const uint64_t fullest = fp.scan_mode ? (uint64_t)n_tris + (shadow ? 0u : in.st_extra) : in.st_maxbin;
    p.shallow = in.st_checked && fullest <= SHALLOW_MAX && !(in.exp.force_deep && !shadow);
    fp.static_div = in.exp.static_div;
    if (!shadow) {   // k_lib_dyn's per-queue lists: every work position could be dynamic
        const size_t n_max = n_owned * (fp.part ? 1 + shs_dev::LIB_MAXK : 1);
        fp.dyn_cap = (uint32_t)((n_max + shs_dev::LIB_NQ - 1) / shs_dev::LIB_NQ + 1);
        p.n_dynq = (size_t)2 * shs_dev::LIB_NQ * fp.dyn_cap;
        fp.heavy_min = (uint32_t)std::max(in.exp.heavy, 0);
    }
    // Camera pass, deep raster: bin lists longer than one candidate round are depth-sorted whole
    // (k_lib_hsort) when the previous pass had such lists (the raster trusts fp.hsort, never the
    // statistics).  Not with k_lib_plan's parts (a part takes a range of list positions).
    fp.hsort = 0u;
    fp.hsort_min = shs_dev::LIB_HSORT_MIN;
#ifndef SHS_EXP_NO_HSORT
    if (!shadow && !fp.scan_mode && !fp.part && !p.shallow && (!in.st_checked || in.st_maxbin > fp.hsort_min)) {
        fp.hsort = 1u;
        p.n_hsq = (size_t)p.n_tiles;
    }
#endif
    // Tile-sharded camera pass in bin mode: each setup workgroup first keeps the rank's triangles of its
    // inputs, positions only (SHS_OPT_SHARD_CULL 0: off).
    p.listed = !shadow && !fp.scan_mode && fp.count > 1 && !fp.reg.on && in.shard_cull;
    // region-sharded camera pass: per setup block its chunk bounds (the next pass's region balance)
    if (!shadow && fp.count > 1 && fp.reg.on) p.n_blkrect = (size_t)p.setup_blocks;
    p.timeline = in.want_timeline && in.timeline_shadow == shadow;
    if (!shadow) {
        p.n_shade = p.n_slots;
        p.n_xbase = (size_t)std::max(n_tris, 1);
        if (p.permuted) p.n_s2s = p.n_xbase;
        if (p.textured) p.n_uvw = 2 * p.n_slots;
        if (p.timeline) p.n_stimeline = (size_t)p.setup_blocks * shs_dev::STL_STRIDE;
        if (in.tm) {   // PassTonemap in k_lib_resolve (shs_lib_fuse_tonemap)
            const size_t npx = (size_t)fp.W * fp.H;
            p.n_tm_thr = 256;
            p.n_tm_ldr = (in.tm->flags & SHS_TONEMAP_LDR) ? npx : 0;
            p.n_tm_present = (in.tm->flags & SHS_TONEMAP_PRESENT) ? npx : 0;
            p.tm_gamma = std::max(0.001f, in.tm->gamma);
            fp.tm_exposure = std::max(0.0001f, in.tm->exposure);
            fp.tm_inv_gamma = 1.0f / p.tm_gamma;
        }
    }
    p.n_tile_count = 2 * (size_t)p.n_tiles;
    p.n_busy = (size_t)p.n_rt;
    p.n_bins = (size_t)p.n_tiles * in.bin_cap;
    p.n_blk_stat = (size_t)p.setup_blocks;
    return p;
}

// The draw table travels with two int32 arrays appended (as whole 16-B-aligned pseudo records): the
// compact tri_base per draw (+ sentinel) and the draw of each setup block's first triangle, so the
// kernels' triangle -> draw lookups start from one load instead of a search over the records.
inline std::vector<LibDrawGPU> build_draw_table(const std::vector<LibDrawGPU> &draws, int setup_blocks) {
    const size_t nd = draws.size();
    const size_t n_int = (nd + 1) + (size_t)setup_blocks;
    const size_t n_extra = (n_int * sizeof(int32_t) + sizeof(LibDrawGPU) - 1) / sizeof(LibDrawGPU);
    std::vector<LibDrawGPU> table(draws);
    table.resize(nd + n_extra);
    int32_t *ints = reinterpret_cast<int32_t *>(table.data() + nd);
    for (size_t i = 0; i < nd; ++i) ints[i] = draws[i].tri_base;
    ints[nd] = (int32_t)lib_pass_tris(draws.data(), nd);
    for (int b = 0, d = 0; b < setup_blocks; ++b) {
        while (d + 1 < (int)nd && draws[d + 1].tri_base <= b * SETUP_BLOCK) ++d;
        ints[nd + 1 + b] = d;
    }
    return table;
}

// k_lib_raster's tile order.  Workgroups b and b + 8 share an XCD (and its L2), and workgroup b
// takes positions b, b + G, ... then tickets of queue b & 7 (positions = q mod 8), so position j
// runs on the XCD j % 8.  Owned bin tiles are grouped into supertiles of st x st bin tiles, the
// supertiles dealt over the 8 XCDs; an XCD's positions walk its supertiles in order, the 4 raster
// rows of a bin tile together.  A primitive's tiles, and a bin tile's 4 rows sharing one bin list,
// then mostly land in one L2 instead of up to eight.  st = 0: the plain order (bin tile, row).
inline std::vector<int32_t> build_rt_order(int tiles_x, int tiles_y, int rtiles_y, int rank, int count, const ShardRegion &reg,
                                           int st) {
    auto owned = [&](int t) { return shs_dev::shard_owned(rank, count, reg, t % tiles_x, t / tiles_x, tiles_x); };
    std::vector<int32_t> out;
    auto push_bt = [&](std::vector<int32_t> &v, int t) {
        const int col = t % tiles_x, brow = t / tiles_x;
        for (int r = 0; r < RT_ROWS; ++r) {
            const int row = brow * RT_ROWS + r;
            if (row < rtiles_y) v.push_back(row * tiles_x + col);
        }
    };
    if (st <= 0) {
        for (int t = 0; t < tiles_x * tiles_y; ++t)
            if (owned(t)) push_bt(out, t);
        return out;
    }
    const int nsx = (tiles_x + st - 1) / st, nsy = (tiles_y + st - 1) / st;
    std::vector<std::vector<int32_t>> lists(8);
    for (int sy = 0; sy < nsy; ++sy)
        for (int sx = 0; sx < nsx; ++sx) {
            std::vector<int32_t> &v = lists[(size_t)((sy * nsx + sx) + 3 * sy) & 7u];
            for (int by = sy * st; by < std::min(tiles_y, (sy + 1) * st); ++by)
                for (int bx = sx * st; bx < std::min(tiles_x, (sx + 1) * st); ++bx) {
                    const int t = by * tiles_x + bx;
                    if (owned(t)) push_bt(v, t);
                }
        }
    size_t longest = 0;
    for (const auto &v : lists) longest = std::max(longest, v.size());
    for (size_t m = 0; m < longest; ++m)
        for (int x = 0; x < 8; ++x)
            if (m < lists[x].size()) out.push_back(lists[x][m]);
    return out;
}

// A footprint shadow pass's tiles: a rectangle of bin tiles and, within it, per bin-tile row y the
// columns x0 | x1 << 16 (x1 < x0: none); an empty span vector: the whole rectangle.
inline void span_cols(uint32_t s, int &x0, int &x1) { x0 = (int)(s & 0xffffu); x1 = (int)(s >> 16); }

// Is every tile of (need, need_span) rendered by (have, have_span)?
inline bool shadow_covers(const ShardRegion &have, const std::vector<uint32_t> &have_span, const ShardRegion &need,
                          const std::vector<uint32_t> &need_span) {
    if (shs_dev::region_empty(need)) return true;
    if (shs_dev::region_empty(have) || need.x0 < have.x0 || need.y0 < have.y0 || need.x1 > have.x1 || need.y1 > have.y1) return false;
    if (have_span.empty()) return true;
    for (int y = need.y0; y <= need.y1; ++y) {
        int a = need.x0, b = need.x1, h0, h1;   // the row's needed columns
        if (!need_span.empty()) {
            if ((size_t)y >= need_span.size()) return false;
            span_cols(need_span[(size_t)y], h0, h1);
            a = std::max(a, h0);
            b = std::min(b, h1);
        }
        if (a > b) continue;
        if ((size_t)y >= have_span.size()) return false;
        span_cols(have_span[(size_t)y], h0, h1);
        if (a < h0 || b > h1) return false;
    }
    return true;
}

// What a pass over both renders: the rectangles' bounding rectangle, the rows' spans united (either
// side without spans, or span vectors of different lengths: the whole rectangle).
inline ShardRegion shadow_union(const ShardRegion &have, const std::vector<uint32_t> &have_span, const ShardRegion &need,
                                const std::vector<uint32_t> &need_span, std::vector<uint32_t> &span) {
    span.clear();
    if (shs_dev::region_empty(have)) {
        span = need_span;
        return need;
    }
    if (!need_span.empty() && need_span.size() == have_span.size()) {
        span.resize(need_span.size());
        for (size_t r = 0; r < span.size(); ++r) {
            int a0, a1, b0, b1;
            span_cols(need_span[r], a0, a1);
            span_cols(have_span[r], b0, b1);
            const bool ea = a1 < a0 || (int)r < need.y0 || (int)r > need.y1;
            const bool eb = b1 < b0 || (int)r < have.y0 || (int)r > have.y1;
            span[r] = ea && eb ? 1u : ea ? have_span[r] : eb ? need_span[r]
                      : (uint32_t)std::min(a0, b0) | ((uint32_t)std::max(a1, b1) << 16);
        }
    }
    return ShardRegion{1, std::min(need.x0, have.x0), std::min(need.y0, have.y0), std::max(need.x1, have.x1),
                       std::max(need.y1, have.y1)};
}

}  // namespace shs_plan
#pragma GCC visibility pop
