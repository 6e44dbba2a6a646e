// shs_abi_shadow.cpp -- PassShadowMap of the library path (include/shs_gpu.h): shs_render_shadow_map, the
// footprint-restricted pass of SHS_OPT_SHADOW_FOOTPRINT (recorded, then enqueued by the camera pass over the
// texels it reads; widened when a later pass reads beyond them) and the map's readback.
// Reference paths are relative to shs-renderer-lib/include/shs/.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/shs_gpu.h"
#include "shs_ctx.hpp"
#include "shs_footprint.hpp"
#include "shs_glm.hpp"
#include "shs_lib_host.hpp"
#include "shs_lib_plan.hpp"

using shs_dev::LibDrawGPU;
using shs_dev::LibFrameParams;
using Work = shs_ctx::LibWork;
using namespace shs_lib_host;

// Enqueue the recorded shadow pass over the bin tiles of `reg` (reg.on = 0: the whole map), within it
// only the row spans `span` (per bin-tile row, x0 | x1 << 16; empty: the whole rectangle).
static int enqueue_shadow(shs_ctx *ctx, const shs_dev::ShardRegion &reg, const std::vector<uint32_t> &span = {}) {
    Work &wk = ctx->lib_shadow;
    wk.last_fp.reg = reg;
    wk.last_fp.rank = 0;
    wk.last_fp.count = reg.on ? 2 : 1;   // a region pass: only the rectangle's tiles are owned
    const bool spans = reg.on && !span.empty() && span.size() <= (size_t)shs_dev::LIB_SPAN_ROWS;
    wk.last_fp.span_rows = spans ? (int32_t)span.size() : 0;
    for (size_t r = 0; spans && r < span.size(); ++r) wk.last_fp.span[r] = span[r];
    ctx->shadow_pending = false;
    ctx->shadow_reg = reg;
    ctx->shadow_span = spans ? span : std::vector<uint32_t>{};
    return enqueue_pass(ctx, wk, true);
}

int shs_lib_flush_shadow(shs_ctx *ctx) {
    if (!ctx->shadow_pending) return SHS_OK;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    return enqueue_shadow(ctx, shs_dev::ShardRegion{0, 0, 0, 0, 0});
}

// A footprint-restricted shadow map whose casters include `pos` (a mesh about to be released) is
// rendered whole first: a later camera pass that reads beyond the footprint could not re-render it.
int shs_lib_widen_shadow(shs_ctx *ctx, const float *pos) {
    if (ctx->shadow_pending || !ctx->have_shadow || !ctx->shadow_reg.on) return SHS_OK;
    bool reads = false;
    for (const LibDrawGPU &d : ctx->lib_shadow.last_draws) reads = reads || d.pos == pos;
    if (!reads) return SHS_OK;
    const int rc = check_superseded(ctx, ctx->lib_shadow);
    return rc ? rc : enqueue_shadow(ctx, shs_dev::ShardRegion{0, 0, 0, 0, 0});
}

// SHS_OPT_SHADOW_FOOTPRINT: the shadow-map bin tiles the camera pass about to be enqueued can read
// (shs_footprint.hpp): the union over its shadowed draws of the light-space bounds of (the draw's world
// box) ∩ (the camera frustum slice of the pixels this rank shades), widened by the PCF reach.
// Also the rows' spans (shs_footprint.hpp footprint_rows, in bin tiles): empty when the map is taller
// than LIB_SPAN_ROWS bin tiles or some draw has no bound.  (-DSHS_SHADOW_SPANS=0: rectangles only,
// a timing comparison.)
#ifndef SHS_SHADOW_SPANS
#define SHS_SHADOW_SPANS 1
#endif
static shs_dev::ShardRegion shadow_region_for(const shs_ctx *ctx, const shs_lib_frame &f, const shs_lib_draw *draws,
                                              int32_t n_draws, const shs_dev::ShardRegion &cam_reg,
                                              std::vector<uint32_t> &span) {
    const int W = f.width, H = f.height;
    int px[4] = {0, 0, W - 1, H - 1};
    if (f.shard_count > 1 && cam_reg.on) {
        px[0] = cam_reg.x0 * shs_dev::TILE;
        px[1] = cam_reg.y0 * shs_dev::TILE;
        px[2] = std::min(W, (cam_reg.x1 + 1) * shs_dev::TILE) - 1;
        px[3] = std::min(H, (cam_reg.y1 + 1) * shs_dev::TILE) - 1;
    }
    const int T = shs_dev::TILE;
    const int rows = (ctx->shadow_h + T - 1) / T;
    bool spans = SHS_SHADOW_SPANS && rows <= shs_dev::LIB_SPAN_ROWS;
    std::vector<int> sx0((size_t)rows, 1), sx1((size_t)rows, 0);   // texel columns per row (x1 < x0: none)
    double pts[220][2];
    shs_fp::TexelRect t;
    for (int i = 0; i < n_draws; ++i) {
        const shs_lib_draw &d = draws[i];
        if (!d.shadow) continue;
        const Mesh &m = ctx->meshes[d.mesh_id];
        double bmin[3], bmax[3];
        shs_fp::world_box(d.model, m.bmin, m.bmax, bmin, bmax);
        const int rad = std::max(0, d.shadow_pcf_radius);
        const int step = std::max(1, (int)std::round((1.0f < d.shadow_pcf_step) ? d.shadow_pcf_step : 1.0f));
        int n_pts = 0;
        t = shs_fp::unite(t, shs_fp::shadow_footprint(d.light_viewproj, ctx->shadow_w, ctx->shadow_h, d.viewproj, W, H, px,
                                                      bmin, bmax, rad * step, pts, &n_pts));
        if (n_pts < 0) spans = false;   // no bound: the whole map
        else if (spans) shs_fp::footprint_rows(pts, n_pts, ctx->shadow_w, ctx->shadow_h, rad * step, T, rows, sx0.data(), sx1.data());
    }
    span.clear();
    if (t.empty()) return shs_dev::ShardRegion{1, 0, 0, -1, -1};
    const shs_dev::ShardRegion reg{1, t.x0 / T, t.y0 / T, t.x1 / T, t.y1 / T};
    if (spans) {
        span.resize((size_t)rows);
        for (int r = 0; r < rows; ++r)
            span[(size_t)r] = sx1[(size_t)r] < sx0[(size_t)r] ? 1u
                              : (uint32_t)(sx0[(size_t)r] / T) | ((uint32_t)(sx1[(size_t)r] / T) << 16);
    }
    return reg;
}

// The shadow map the camera pass about to be enqueued samples: the recorded pass, narrowed to what this
// pass reads; or a map rendered for an earlier camera pass's footprint, sampled again (a static sun
// reused over frames, another view or region) -- the texels this pass reads must lie inside what was
// rendered, or the pass is enqueued again over the union (stream-ordered after the earlier camera
// passes; re-rendered texels get the same values).
int shs_lib_host::shadow_for_camera(shs_ctx *ctx, const shs_lib_frame &f, const shs_lib_draw *draws, int32_t n_draws,
                                    const shs_dev::ShardRegion &cam_reg) {
    std::vector<uint32_t> span;
    if (ctx->shadow_pending) {
        const shs_dev::ShardRegion need = shadow_region_for(ctx, f, draws, n_draws, cam_reg, span);
        return enqueue_shadow(ctx, need, span);
    }
    if (!ctx->have_shadow || !ctx->shadow_reg.on) return SHS_OK;
    bool shadowed = false;
    for (int i = 0; i < n_draws; ++i) shadowed = shadowed || draws[i].shadow;
    if (!shadowed) return SHS_OK;
    const shs_dev::ShardRegion need = shadow_region_for(ctx, f, draws, n_draws, cam_reg, span);
    const shs_dev::ShardRegion have = ctx->shadow_reg;
    const std::vector<uint32_t> have_span = ctx->shadow_span;
    if (shs_plan::shadow_covers(have, have_span, need, span)) return SHS_OK;
    std::vector<uint32_t> us;
    const shs_dev::ShardRegion u = shs_plan::shadow_union(have, have_span, need, span, us);
    const int rc = check_superseded(ctx, ctx->lib_shadow);
    return rc ? rc : enqueue_shadow(ctx, u, us);
}

extern "C" {

int shs_render_shadow_map(shs_ctx *ctx, int32_t w, int32_t h, const float sun_dir[3], const shs_shadow_caster *casters,
                          int32_t n_casters, float light_viewproj_out[16]) {
    if (!ctx || !sun_dir || w <= 0 || h <= 0 || w > 16384 || h > 16384 || n_casters < 0 || (n_casters > 0 && !casters))
        return SHS_ERR_INVALID;
    for (int i = 0; i < n_casters; ++i)
        if (check_lib_mesh(ctx, casters[i].mesh_id)) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    if (!ctx->h_lib_counters && hipHostMalloc(reinterpret_cast<void **>(&ctx->h_lib_counters), shs_dev::LC_N * sizeof(uint32_t)) != hipSuccess)
        return SHS_ERR_HIP;
    {   // the pending passes are checked before this one rewrites the shadow map they read / wrote
        const int rc = check_superseded(ctx, ctx->lib_shadow);
        if (rc) return rc;
        const int rc2 = check_superseded(ctx, ctx->lib_cam);
        if (rc2) return rc2;
    }
    using namespace shs_host;
    // scene AABB of the casters (pass_shadow_map.hpp:80-131)
    vec3 mn = {1e30f, 1e30f, 1e30f}, mx = {-1e30f, -1e30f, -1e30f};
    auto expand = [&](vec3 p) {
        mn = {(p.x < mn.x) ? p.x : mn.x, (p.y < mn.y) ? p.y : mn.y, (p.z < mn.z) ? p.z : mn.z};
        mx = {(mx.x < p.x) ? p.x : mx.x, (mx.y < p.y) ? p.y : mx.y, (mx.z < p.z) ? p.z : mx.z};
    };
    bool any = false;
    for (int i = 0; i < n_casters; ++i) {
        const Mesh &m = ctx->meshes[casters[i].mesh_id];
        const float *b0 = m.bmin, *b1 = m.bmax, *M = casters[i].model;
        const vec3 c[8] = {{b0[0], b0[1], b0[2]}, {b1[0], b0[1], b0[2]}, {b0[0], b1[1], b0[2]}, {b1[0], b1[1], b0[2]},
                           {b0[0], b0[1], b1[2]}, {b1[0], b0[1], b1[2]}, {b0[0], b1[1], b1[2]}, {b1[0], b1[1], b1[2]}};
        for (const vec3 &p : c)
            expand(vec3{(M[0] * p.x + M[4] * p.y) + (M[8] * p.z + M[12] * 1.0f), (M[1] * p.x + M[5] * p.y) + (M[9] * p.z + M[13] * 1.0f),
                        (M[2] * p.x + M[6] * p.y) + (M[10] * p.z + M[14] * 1.0f)});
        any = true;
    }
    if (!any) { expand(vec3{-1.0f, -1.0f, -1.0f}); expand(vec3{1.0f, 1.0f, 1.0f}); }
    float view[16], proj[16];
    dir_light_camera_aabb(vec3{sun_dir[0], sun_dir[1], sun_dir[2]}, mn, mx, 10.0f, (uint32_t)std::max(w, 1), view, proj,
                          ctx->shadow_vp);
    if (light_viewproj_out) std::memcpy(light_viewproj_out, ctx->shadow_vp, sizeof ctx->shadow_vp);

    if (ensure(ctx, ctx->shadow_map, (size_t)w * h)) return SHS_ERR_HIP;
    Work &wk = ctx->lib_shadow;
    wk.last_draws.clear();
    int32_t base = 0;
    for (int i = 0; i < n_casters; ++i) {
        const Mesh &m = ctx->meshes[casters[i].mesh_id];
        LibDrawGPU d;
        std::memset(&d, 0, sizeof d);
        d.pos = m.pos; d.nrm = m.nrm; d.uv = m.uv; d.idx = m.idx;
        d.n_verts = m.n_verts; d.tri_base = base; d.n_tris = m.n_tris;
        std::memcpy(d.model, casters[i].model, sizeof d.model);
        std::memcpy(d.viewproj, ctx->shadow_vp, sizeof d.viewproj);
        wk.last_draws.push_back(d);
        base += m.n_tris;
    }
    LibFrameParams fp;
    std::memset(&fp, 0, sizeof fp);
    fp.W = w; fp.H = h;
    fp.rank = 0; fp.count = 1;   // the whole shadow map (SHS_OPT_SHADOW_FOOTPRINT: the next camera pass narrows it)
    wk.last_fp = fp;
    ctx->shadow_w = w;
    ctx->shadow_h = h;
    ctx->cam_after_shadow = false;
    ctx->have_shadow = true;
    if (ctx->shadow_footprint) {   // recorded; shs_render_pbr_forward enqueues it for the texels it reads
        ctx->shadow_pending = true;
        return SHS_OK;
    }
    ctx->shadow_pending = false;
    ctx->shadow_reg = shs_dev::ShardRegion{0, 0, 0, 0, 0};
    ctx->shadow_span.clear();
    return enqueue_pass(ctx, wk, true);
}

int shs_get_shadow_region(shs_ctx *ctx, int32_t rect[4]) {
    if (!ctx || !rect) return SHS_ERR_INVALID;
    if (!ctx->have_shadow) { ctx->err = "no shadow map rendered"; return SHS_ERR_INVALID; }
    const shs_dev::ShardRegion &g = ctx->shadow_reg;
    const int tx = (ctx->shadow_w + shs_dev::TILE - 1) / shs_dev::TILE, ty = (ctx->shadow_h + shs_dev::TILE - 1) / shs_dev::TILE;
    if (ctx->shadow_pending) { rect[0] = 1; rect[1] = 1; rect[2] = 0; rect[3] = 0; return SHS_OK; }
    rect[0] = g.on ? g.x0 : 0; rect[1] = g.on ? g.y0 : 0;
    rect[2] = g.on ? g.x1 : tx - 1; rect[3] = g.on ? g.y1 : ty - 1;
    return SHS_OK;
}

int shs_shadow_footprint(const float light_viewproj[16], int32_t sm_w, int32_t sm_h, const float camera_viewproj[16],
                         int32_t width, int32_t height, const int32_t px_rect[4], const float world_min[3],
                         const float world_max[3], int32_t reach, int32_t texel_rect[4]) {
    if (!light_viewproj || !camera_viewproj || !px_rect || !world_min || !world_max || !texel_rect || reach < 0)
        return SHS_ERR_INVALID;
    const int px[4] = {px_rect[0], px_rect[1], px_rect[2], px_rect[3]};
    const double b0[3] = {world_min[0], world_min[1], world_min[2]}, b1[3] = {world_max[0], world_max[1], world_max[2]};
    const shs_fp::TexelRect t = shs_fp::shadow_footprint(light_viewproj, sm_w, sm_h, camera_viewproj, width, height, px, b0, b1, reach);
    texel_rect[0] = t.x0; texel_rect[1] = t.y0; texel_rect[2] = t.x1; texel_rect[3] = t.y1;
    return SHS_OK;
}

int shs_shadow_footprint_rows(const float light_viewproj[16], int32_t sm_w, int32_t sm_h, const float camera_viewproj[16],
                              int32_t width, int32_t height, const int32_t px_rect[4], const float world_min[3],
                              const float world_max[3], int32_t reach, int32_t row_h, int32_t n_rows, int32_t *x0,
                              int32_t *x1) {
    if (!light_viewproj || !camera_viewproj || !px_rect || !world_min || !world_max || !x0 || !x1 || reach < 0 ||
        row_h <= 0 || n_rows < 0)
        return SHS_ERR_INVALID;
    const int px[4] = {px_rect[0], px_rect[1], px_rect[2], px_rect[3]};
    const double b0[3] = {world_min[0], world_min[1], world_min[2]}, b1[3] = {world_max[0], world_max[1], world_max[2]};
    double pts[220][2];
    int n_pts = 0;
    shs_fp::shadow_footprint(light_viewproj, sm_w, sm_h, camera_viewproj, width, height, px, b0, b1, reach, pts, &n_pts);
    for (int r = 0; r < n_rows; ++r) {
        x0[r] = n_pts < 0 ? 0 : 1;
        x1[r] = n_pts < 0 ? sm_w - 1 : 0;
    }
    if (n_pts > 0) shs_fp::footprint_rows(pts, n_pts, sm_w, sm_h, reach, row_h, n_rows, x0, x1);
    return SHS_OK;
}

int shs_resolve_shadow_map(shs_ctx *ctx, float *depth) {
    if (!ctx || !depth) return SHS_ERR_INVALID;
    if (!ctx->have_shadow) { ctx->err = "no shadow map rendered"; return SHS_ERR_INVALID; }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    int rc = shs_lib_flush_shadow(ctx);   // a recorded footprint pass is rendered whole for a readback
    if (rc) return rc;
    rc = lib_finish(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(depth, ctx->shadow_map.p, (size_t)ctx->shadow_w * ctx->shadow_h * sizeof(float), hipMemcpyDeviceToHost));
    return SHS_OK;
}

}  // extern "C"
