// shs_abi_lib.cpp -- the pass machinery of the library raster path of libshs_gpu.so (include/shs_gpu.h,
// "Library path"): a pass is planned (shs_lib_plan.hpp), then sized, bound and launched here, and re-issued
// when a capacity overflowed; PassPBRForward (rasterize_mesh per item) and the resolves.  PassShadowMap:
// shs_abi_shadow.cpp; meshes and textures: shs_abi_mesh.cpp; sky: shs_abi_sky.cpp; light lists:
// shs_abi_light_cull.cpp.  Reference paths are relative to shs-renderer-lib/include/shs/.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/shs_gpu.h"
#include "shs_ctx.hpp"
#include "shs_glm.hpp"
#include "shs_lib_device.hpp"
#include "shs_lib_host.hpp"
#include "shs_lib_internal.hpp"
#include "shs_lib_plan.hpp"

using shs_dev::LibBuffers;
using shs_dev::LibDrawGPU;
using shs_dev::LibFrameParams;
using shs_plan::LibPassPlan;
using Work = shs_ctx::LibWork;
using namespace shs_lib_host;

static_assert(shs_plan::BIN_TILE == shs_dev::TILE, "the plan's bin tile is the kernels'");

namespace {

int harvest(shs_ctx *ctx, Work &w, int k) {
    if (!w.ring_pending[k]) return SHS_OK;
    HIP_TRY(ctx, hipEventSynchronize(w.ring_ev[k][2]));
    float a = 0.0f, b = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&a, w.ring_ev[k][0], w.ring_ev[k][1]));
    HIP_TRY(ctx, hipEventElapsedTime(&b, w.ring_ev[k][1], w.ring_ev[k][2]));
    w.acc_ms[0] += a;
    w.acc_ms[1] += b;
    w.acc_n++;
    w.ring_pending[k] = false;
    return SHS_OK;
}

int harvest_all(shs_ctx *ctx, Work &w) {
    for (int j = 0; j < Work::RING; ++j)
        if (harvest(ctx, w, (w.ring_next + j) % Work::RING)) return SHS_ERR_HIP;
    return SHS_OK;
}

void release_work(Work &w) {
    for (auto &ev : w.ring_ev)
        for (auto &e : ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
    release(w.draws); release(w.recs); release(w.shade); release(w.boxes); release(w.xbase); release(w.zord); release(w.s2s); release(w.blist);
    w.dev_table.clear();
    w.dev_table_at = nullptr;
    w.dev_table_cap = 0;
    release(w.tile_count); release(w.bins); release(w.counters); release(w.busy);
    release(w.spill); release(w.blk_stat); release(w.rstat); release(w.uvw); release(w.items); release(w.pkeys); release(w.pcount); release(w.dynq); release(w.hsq); release(w.hsr); release(w.clipq); release(w.bigq); release(w.bigpre); release(w.rqueue);
    if (w.raster_ev) (void)hipEventDestroy(w.raster_ev);
    if (w.resolve_ev) (void)hipEventDestroy(w.resolve_ev);
    w.raster_ev = w.resolve_ev = nullptr;
    if (w.ov_after) (void)hipEventDestroy(w.ov_after);
    if (w.h_ov) (void)hipHostFree(const_cast<uint32_t *>(w.h_ov));
    if (w.h_blkrect) (void)hipHostFree(w.h_blkrect);
    w.h_blkrect = nullptr;
    w.blkrect_cap = 0;
    w.blkrect_valid = false;
    w.ov_after = nullptr;
    w.h_ov = nullptr;
    w.ov_valid = false;
    w.resolve_ev_valid = false;
    for (int i = 0; i < 2; ++i) {
        if (w.h_draws[i]) (void)hipHostFree(w.h_draws[i]);
        if (w.slot_ev[i]) (void)hipEventDestroy(w.slot_ev[i]);
        w.h_draws[i] = nullptr;
        w.slot_ev[i] = nullptr;
    }
}

// Per-draw block: the uniform-only products of the reference's per-vertex / per-fragment code,
// computed once with the same float operations (shs_glm.hpp restates GLM's op order).
void build_lib_draw(const shs_lib_draw &in, const Mesh &m, int32_t base, LibDrawGPU &o) {
    using namespace shs_host;
    std::memset(&o, 0, sizeof o);
    o.pos = m.pos; o.nrm = m.nrm; o.uv = m.uv; o.idx = m.idx;
    o.cbox = m.cbox;
    o.orig = m.orig;
    o.n_verts = m.n_verts;
    o.tri_base = base;
    o.n_tris = m.n_tris;
    o.program = in.program;
    o.cull_mode = in.cull_mode;
    o.front_ccw = in.front_face_ccw != 0;
    o.shadow = in.shadow != 0;
    o.motion = in.enable_motion_vectors != 0;
    std::memcpy(o.model, in.model, sizeof o.model);
    std::memcpy(o.viewproj, in.viewproj, sizeof o.viewproj);
    lib_normal_matrix(in.model, o.nmat);                       // builtin_shaders.hpp:93-95
    if (std::fabs(det4(in.model)) > 1e-10f) {                  // rasterizer.hpp:296-308
        float inv[16];
        inverse(in.model, inv);
        mul(in.prev_model, inv, o.c2p);
    } else {
        identity(o.c2p);
    }
    std::memcpy(o.prev_vp, in.prev_viewproj, sizeof o.prev_vp);
    std::memcpy(o.light_vp, in.light_viewproj, sizeof o.light_vp);
    const vec3 L = gnormalize(gneg(vec3{in.light_dir_ws[0], in.light_dir_ws[1], in.light_dir_ws[2]}));
    o.L[0] = L.x; o.L[1] = L.y; o.L[2] = L.z;
    for (int i = 0; i < 3; ++i) {
        o.cam[i] = in.camera_pos[i];
        o.lcol[i] = in.light_color[i];
        o.base[i] = in.base_color[i];
    }
    o.lcol[3] = in.light_intensity;
    o.base[3] = in.metallic;
    o.mat[0] = in.roughness;
    o.mat[1] = in.ao;
    o.mat[2] = in.shadow_strength;
    // ShadowParams as the builtin FS builds them: pcf_radius = max(0, r), pcf_step = max(1, step)
    o.shp[0] = in.shadow_bias_const;
    o.shp[1] = in.shadow_bias_slope;
    const int32_t rad = std::max(0, in.shadow_pcf_radius);
    std::memcpy(&o.shp[2], &rad, sizeof rad);
    o.shp[3] = (1.0f < in.shadow_pcf_step) ? in.shadow_pcf_step : 1.0f;
}

// u.base_color_tex (pass_pbr_forward.hpp:173-176): texture id k >= 1, 0 = none.
void bind_texture(const shs_ctx *ctx, int32_t id, LibDrawGPU &o) {
    if (id <= 0) return;
    const Texture &t = ctx->textures[(size_t)id - 1];
    o.tex = t.texels;
    o.tex_w = t.w;
    o.tex_h = t.h;
}

// Upload the draw table through the work's pinned 2-slot staging.  A table equal to the one the
// device buffer already holds (a prepared pass re-rendered) is not sent again: the stream-ordered copy
// is a DMA between two kernels, ~20 us of idle GPU per frame.
int upload_draws(shs_ctx *ctx, Work &w, const std::vector<LibDrawGPU> &d, hipStream_t st) {
    const size_t n = std::max<size_t>(d.size(), 1);
    if (ensure(ctx, w.draws, n)) return SHS_ERR_HIP;
    if (w.dev_table_at == w.draws.p && w.dev_table_cap == w.draws.cap && w.dev_table.size() == d.size() &&
        (d.empty() || std::memcmp(w.dev_table.data(), d.data(), d.size() * sizeof(LibDrawGPU)) == 0))
        return SHS_OK;
    const int s = w.slot;
    w.slot ^= 1;
    if (!w.slot_ev[0])
        for (int i = 0; i < 2; ++i) HIP_TRY(ctx, hipEventCreateWithFlags(&w.slot_ev[i], hipEventDisableTiming));
    if (w.slot_used[s]) HIP_TRY(ctx, hipEventSynchronize(w.slot_ev[s]));
    if (n > w.h_cap) {
        for (int i = 0; i < 2; ++i) {
            if (i != s && w.slot_used[i]) HIP_TRY(ctx, hipEventSynchronize(w.slot_ev[i]));
            if (w.h_draws[i]) HIP_TRY(ctx, hipHostFree(w.h_draws[i]));
            w.h_draws[i] = nullptr;
        }
        const size_t cap = std::max<size_t>(n, 16);
        for (int i = 0; i < 2; ++i) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&w.h_draws[i]), cap * sizeof(LibDrawGPU)));
        w.h_cap = cap;
    }
    if (!d.empty()) {
        std::memcpy(w.h_draws[s], d.data(), d.size() * sizeof(LibDrawGPU));
        HIP_TRY(ctx, hipMemcpyAsync(w.draws.p, w.h_draws[s], d.size() * sizeof(LibDrawGPU), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ctx, hipEventRecord(w.slot_ev[s], st));
    w.slot_used[s] = true;
    w.dev_table = d;
    w.dev_table_at = w.draws.p;
    w.dev_table_cap = w.draws.cap;
    return SHS_OK;
}

// The raster tile order (shs_lib_plan.hpp build_rt_order) of this geometry and ownership, cached.
int rt_order_for(shs_ctx *ctx, const LibFrameParams &fp, int st, const shs_ctx::OrderEntry *&order) {
    const int tiles_x = (fp.W + shs_dev::TILE - 1) / shs_dev::TILE, tiles_y = (fp.H + shs_dev::TILE - 1) / shs_dev::TILE;
    const int rtiles_y = (fp.H + 7) / 8;
    const shs_dev::ShardRegion reg = fp.count > 1 ? fp.reg : shs_dev::ShardRegion{0, 0, 0, 0, 0};
    const int rank = fp.count > 1 ? fp.rank : 0, count = std::max(fp.count, 1);
    const uint64_t key[4] = {(uint64_t)tiles_x | ((uint64_t)tiles_y << 16) | ((uint64_t)rtiles_y << 32) | ((uint64_t)(st & 0xff) << 56),
                             (uint64_t)(uint32_t)rank | ((uint64_t)(uint32_t)count << 32), region_key(reg), (uint64_t)reg.on};
    if ((order = order_find(ctx->rt_orders, key))) return SHS_OK;
    const std::vector<int32_t> v = shs_plan::build_rt_order(tiles_x, tiles_y, rtiles_y, rank, count, reg, st);
    return order_insert(ctx, ctx->rt_orders, key, v, (int)v.size(), order);
}

// The experiments build's overrides of a plan (the product build reads no environment): the per-pass
// switches on every call, the others once per process.
shs_plan::LibPlanExp plan_overrides() {
    shs_plan::LibPlanExp x;
    if (const char *e = shs_exp_env("SHS_LIB_XCD_ST")) x.xcd_st = (int)std::strtol(e, nullptr, 0);
    if (const char *e = shs_exp_env("SHS_LIB_SCAN_MAX")) x.scan_max = std::strtol(e, nullptr, 0);
    if (const char *e = shs_exp_env("SHS_LIB_EXP")) x.exp_flags = (uint32_t)std::strtoul(e, nullptr, 0);
    static const shs_plan::LibPlanExp once = [] {
        shs_plan::LibPlanExp o;
        if (const char *e = shs_exp_env("SHS_LIB_DEEP")) o.force_deep = std::atoi(e);
        if (const char *e = shs_exp_env("SHS_LIB_STATIC_DIV")) o.static_div = std::atoi(e);
        if (const char *e = shs_exp_env("SHS_LIB_HEAVY")) o.heavy = std::atoi(e);
        return o;
    }();
    x.force_deep = once.force_deep;
    x.static_div = once.static_div;
    x.heavy = once.heavy;
    return x;
}

// Every allocation the plan asks for, and the stream operations that go with a (re)allocation: the
// per-tile state's zeroing on a geometry change, the draw table's upload, the split tiles' key slots'
// first fill, the timelines' zeroing.
int size_lib_pass(shs_ctx *ctx, Work &w, const LibPassPlan &p, const std::vector<LibDrawGPU> &table, int raster_grid,
                  hipStream_t ps) {
    auto opt = [&](auto &buf, size_t n) { return n ? ensure(ctx, buf, n) : (int)SHS_OK; };
    // every slot enters the large-primitive queue at most once
    if (ensure(ctx, w.recs, p.n_slots) || ensure(ctx, w.boxes, p.n_slots) || ensure(ctx, w.zord, p.n_slots) ||
        ensure(ctx, w.bigq, p.n_slots) || ensure(ctx, w.bigpre, p.n_slots))
        return SHS_ERR_HIP;
    if (opt(w.shade, p.n_shade) || opt(w.xbase, p.n_xbase) || opt(w.clipq, p.n_xbase) || opt(w.s2s, p.n_s2s) || opt(w.uvw, p.n_uvw))
        return SHS_ERR_HIP;
    if (p.n_uvw && ensure_srgb_lut(ctx)) return SHS_ERR_HIP;
    const bool reset = p.geom_key != w.geom_key || p.rtiles_y != w.geom_rtiles_y || w.tile_count.cap < p.n_tile_count ||
                       w.busy.cap < p.n_busy || !w.counters.p;
    if (ensure(ctx, w.tile_count, p.n_tile_count) || ensure(ctx, w.busy, p.n_busy) || ensure(ctx, w.counters, 2 * shs_dev::LC_N) ||
        ensure(ctx, w.rqueue, 2 * shs_dev::LIB_NQW * shs_dev::LIB_QSTRIDE))
        return SHS_ERR_HIP;
    if (reset) {
        HIP_TRY(ctx, hipMemsetAsync(w.tile_count.p, 0, w.tile_count.cap * sizeof(uint32_t), ps));
        HIP_TRY(ctx, hipMemsetAsync(w.busy.p, 0, w.busy.cap * sizeof(uint32_t), ps));
        HIP_TRY(ctx, hipMemsetAsync(w.counters.p, 0, w.counters.cap * sizeof(uint32_t), ps));
        HIP_TRY(ctx, hipMemsetAsync(w.rqueue.p, 0, w.rqueue.cap * sizeof(uint32_t), ps));
        w.geom_key = p.geom_key;
        w.geom_rtiles_y = p.rtiles_y;
    }
    if (ensure(ctx, w.bins, p.n_bins) || ensure(ctx, w.blk_stat, p.n_blk_stat) || ensure(ctx, w.rstat, (size_t)raster_grid) ||
        opt(w.items, p.n_items) || opt(w.dynq, p.n_dynq) || opt(w.hsq, p.n_hsq) || opt(w.hsr, p.n_hsq) || opt(w.blist, p.n_blkrect))
        return SHS_ERR_HIP;
    if (upload_draws(ctx, w, table, ps)) return SHS_ERR_HIP;
    if (w.pkeys.cap < p.n_pkeys || w.pcount.cap < p.n_pcount) {   // KEY_EMPTY / 0 once, then reset by each tile's last part
        if (ensure(ctx, w.pkeys, p.n_pkeys) || ensure(ctx, w.pcount, p.n_pcount)) return SHS_ERR_HIP;
        HIP_TRY(ctx, hipMemsetAsync(w.pkeys.p, 0xff, w.pkeys.cap * sizeof(unsigned long long), ps));
        HIP_TRY(ctx, hipMemsetAsync(w.pcount.p, 0, w.pcount.cap * sizeof(uint32_t), ps));
    }
    if (p.n_blkrect) {   // the block bounds, in mapped host memory (the next pass's region balance reads them)
        if (p.n_blkrect > w.blkrect_cap) {
            if (w.h_blkrect) {
                if (w.ov_valid) HIP_TRY(ctx, hipEventSynchronize(w.ov_after));
                HIP_TRY(ctx, hipHostFree(w.h_blkrect));
                w.h_blkrect = nullptr;
            }
            const size_t cap = std::max<size_t>(p.n_blkrect, 1024);
            HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&w.h_blkrect), cap * sizeof(uint4),
                                       hipHostMallocMapped | hipHostMallocCoherent));
            w.blkrect_cap = cap;
        }
        w.blkrect_n = p.setup_blocks;
        w.blkrect_w = p.fp.W;
        w.blkrect_h = p.fp.H;
        w.blkrect_valid = true;
    }
    if (opt(ctx->lib_ldr, p.n_tm_ldr) || opt(ctx->lib_present, p.n_tm_present) || opt(ctx->tm_thr_dev, p.n_tm_thr)) return SHS_ERR_HIP;
    if (p.n_tm_thr && ctx->tm_thr_dev_gamma != p.tm_gamma) {   // rare (a new gamma): a synchronous upload
        float thr[256];
        shs_tonemap_thresholds(p.tm_gamma, thr);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(ctx->tm_thr_dev.p, thr, sizeof thr, hipMemcpyHostToDevice));
        ctx->tm_thr_dev_gamma = p.tm_gamma;
    }
    if (p.timeline) {   // (profiling: the raster's workgroups, the camera pass's setup workgroups)
        const size_t n = (size_t)raster_grid * shs_dev::LTL_STRIDE;
        if (ensure(ctx, ctx->lib_timeline, n)) return SHS_ERR_HIP;
        HIP_TRY(ctx, hipMemsetAsync(ctx->lib_timeline.p, 0, n * sizeof(uint64_t), ps));
        if (p.n_stimeline) {
            if (ensure(ctx, ctx->lib_stimeline, p.n_stimeline)) return SHS_ERR_HIP;
            HIP_TRY(ctx, hipMemsetAsync(ctx->lib_stimeline.p, 0, p.n_stimeline * sizeof(uint64_t), ps));
        }
    }
    return SHS_OK;
}

// The kernels' buffer table of a sized pass: each optional pointer next to the plan field that enables it.
void bind_lib_pass(const shs_ctx *ctx, const Work &w, const LibPassPlan &p, bool shadow, const shs_ctx::OrderEntry &order,
                   LibBuffers &fb) {
    std::memset(&fb, 0, sizeof fb);
    fb.draws = w.draws.p; fb.recs = w.recs.p; fb.shade = w.shade.p; fb.boxes = w.boxes.p; fb.xbase = w.xbase.p; fb.zord = w.zord.p;
    fb.tile_count = w.tile_count.p; fb.bins = w.bins.p; fb.spill = w.spill.p; fb.counters = w.counters.p;
    fb.busy = w.busy.p; fb.blk_stat = w.blk_stat.p; fb.rstat = w.rstat.p;
    fb.clipq = w.clipq.p; fb.bigq = w.bigq.p; fb.bigpre = w.bigpre.p;
    fb.dbase = reinterpret_cast<int32_t *>(w.draws.p + p.fp.n_draws);
    fb.bdraw = fb.dbase + p.fp.n_draws + 1;
    fb.rqueue = w.rqueue.p;
    fb.rt_order = order.dev;
    fb.ov_host = const_cast<uint32_t *>(w.h_ov);
    if (p.n_s2s) fb.s2s = w.s2s.p;
    if (p.n_dynq) fb.dynq = w.dynq.p;
    if (p.n_items) { fb.items = w.items.p; fb.pkeys = w.pkeys.p; fb.pcount = w.pcount.p; }
    if (p.n_hsq) { fb.hsq = w.hsq.p; fb.hsr = w.hsr.p; }
    if (p.n_blkrect) { fb.blkrect = w.h_blkrect; fb.blist = w.blist.p; }
    if (p.timeline) fb.timeline = ctx->lib_timeline.p;
    if (p.n_stimeline) fb.stimeline = ctx->lib_stimeline.p;
    if (shadow) {
        fb.depth = ctx->shadow_map.p;
        return;
    }
    fb.hdr = ctx->lib_hdr.p; fb.depth = ctx->lib_depth.p; fb.motion = ctx->lib_motion.p;
    fb.keys = ctx->lib_keys.p;
    fb.blkcov = ctx->lib_blkcov.p;
    if (p.n_uvw) fb.uvw = w.uvw.p;
    fb.srgb_lut = ctx->srgb_lut.p;
    if (p.n_tm_thr) fb.tm_thr = ctx->tm_thr_dev.p;   // PassTonemap in k_lib_resolve (shs_lib_fuse_tonemap)
    if (p.n_tm_ldr) fb.tm_ldr = ctx->lib_ldr.p;
    if (p.n_tm_present) fb.tm_present = ctx->lib_present.p;
    fb.shadow_map = ctx->have_shadow ? ctx->shadow_map.p : nullptr;
    fb.lights = ctx->lights.p;
    fb.tlights = ctx->lights_typed ? ctx->tlights.p : nullptr;
    fb.tile_counts = ctx->list_counts.p;
    fb.tile_indices = ctx->list_indices.p;
}

// The pass's kernels on `ps` (the camera pass's resolve on the context's stream), between the timing
// ring's events; the overflow word is zeroed before, the re-issue bookkeeping updated after.
int launch_lib_pass(shs_ctx *ctx, Work &w, const LibPassPlan &p, const LibBuffers &fb, bool shadow, int raster_grid, int resolve_grid,
                    hipStream_t ps) {
    const LibFrameParams &fp = p.fp;
    hipEvent_t *ev = nullptr;
    if (ctx->timing) {
        const int k = w.ring_next;
        w.ring_next = (k + 1) % Work::RING;
        if (harvest(ctx, w, k)) return SHS_ERR_HIP;
        if (!w.ring_ev[k][0])
            for (int i = 0; i < 3; ++i) HIP_TRY(ctx, hipEventCreateWithFlags(&w.ring_ev[k][i], hipEventDisableSystemFence));
        ev = w.ring_ev[k];
        w.ring_pending[k] = true;
    }
    // the previous pass's setup (the only other writer of the word) is done before it is zeroed
    if (w.ov_valid) HIP_TRY(ctx, hipEventSynchronize(w.ov_after));
    *w.h_ov = 0u;
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[0], ps));
    HIP_TRY(ctx, shs_internal::launch_lib_setup(fp, fb, shadow, p.listed, ps));
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[1], ps));
    // the pass's overflow word is final after its setup kernels (setup, clip, large-primitive marks), so
    // superseding the pass checks it at ov_after, without waiting for the raster
    HIP_TRY(ctx, hipEventRecord(w.ov_after, ps));
    w.ov_valid = true;
    HIP_TRY(ctx, shs_internal::launch_lib_raster(fp, fb, shadow, p.shallow, raster_grid, ps));
    if (!shadow) {   // the camera pass's shading runs in its own kernel (event [2] closes both)
        if (ps != ctx->stream) {
            HIP_TRY(ctx, hipEventRecord(w.raster_ev, ps));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, w.raster_ev, 0));
        }
        HIP_TRY(ctx, shs_internal::launch_lib_resolve(fp, fb, p.prog, p.wide, resolve_grid, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(w.resolve_ev, ctx->stream));
        w.resolve_ev_valid = true;
    }
    if (ev) HIP_TRY(ctx, hipEventRecord(ev[2], ctx->stream));
    w.last_parity = fp.parity;
    w.frame_index++;
    w.last_setup_blocks = shs_internal::lib_setup_grid(fp.n_tris, p.listed);
    w.last_raster_grid = raster_grid;
    w.last_n_tris = fp.n_tris;
    w.need_check = true;
    w.done = true;
    return SHS_OK;
}

}  // namespace

// Enqueue one pass (w.last_fp / w.last_draws describe it): plan it, size its workspace, bind and launch.
// shadow: PassShadowMap's depth pass into ctx->shadow_map.
int shs_lib_host::enqueue_pass(shs_ctx *ctx, Work &w, bool shadow) {
    if (shs_plan::lib_pass_tris(w.last_draws.data(), w.last_draws.size()) > shs_plan::MAX_PASS_TRIS) {
        ctx->err = "too many triangles in one pass";
        return SHS_ERR_INVALID;
    }
    if (!w.spill.p && ensure(ctx, w.spill, 1 << 16)) return SHS_ERR_HIP;   // (the plan reads its capacity)
    if (!w.ov_after) {
        HIP_TRY(ctx, hipEventCreateWithFlags(&w.ov_after, hipEventDisableTiming));
        HIP_TRY(ctx, shs_host_ov_alloc(&w.h_ov));
    }
    shs_plan::LibPassInputs in;
    in.shadow = shadow;
    in.desc = &w.last_fp;
    in.draws = w.last_draws.data();
    in.n_draws = w.last_draws.size();
    in.tm = (!shadow && w.tm_fused) ? &w.tm_desc : nullptr;
    in.st_checked = w.st_checked; in.st_maxbin = w.st_maxbin; in.st_extra = w.st_extra;
    in.bin_cap = w.bin_cap; in.extra_cap = w.extra_cap; in.frame_index = w.frame_index;
    in.spill_cap = w.spill.cap;
    in.lib_part = ctx->lib_part; in.shard_cull = ctx->shard_cull; in.cam_after_shadow = ctx->cam_after_shadow;
    in.want_timeline = ctx->want_timeline; in.timeline_shadow = ctx->timeline_shadow;
    in.exp = plan_overrides();
    const shs_ctx::OrderEntry *order = nullptr;
    if (rt_order_for(ctx, w.last_fp, in.exp.xcd_st, order)) return SHS_ERR_HIP;
    in.n_owned_rt = order->n;
    LibPassPlan plan = shs_plan::plan_lib_pass(in);
    w.extra_cap = plan.extra_cap;

    // With ctx->cam_after_shadow (timing experiments only since round 6, SHS_EXP_CAM_SIDE_STREAM) the camera
    // pass's setup and raster run on the side stream (ctx->setup_stream) beside the shadow pass on the main
    // stream; they read only the meshes and the draw table, and wait for the previous camera resolve (it
    // reads the records, the draw table and the keys this pass rewrites); the resolve waits for the raster.
    hipStream_t ps = plan.side_stream ? ctx->setup_stream : ctx->stream;
    if (!shadow) {
        if (!w.raster_ev) {
            HIP_TRY(ctx, hipEventCreateWithFlags(&w.raster_ev, hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&w.resolve_ev, hipEventDisableTiming));
        }
        if (w.resolve_ev_valid && ps != ctx->stream) HIP_TRY(ctx, hipStreamWaitEvent(ps, w.resolve_ev, 0));
    }
    int &resident = ctx->lib_resident[shadow ? 1 : 0][plan.shallow ? 1 : 0];
    if (resident <= 0) resident = shs_internal::lib_raster_resident_blocks(ctx->device, shadow, plan.shallow);
    const int raster_grid = plan.fp.raster_grid = std::max(1, std::min(plan.fp.n_owned_rt, resident));
    int resolve_grid = 0;
    if (!shadow) {
        int &res = ctx->lib_resolve_resident[shs_plan::resolve_variant(plan.prog, plan.wide, plan.sky)];
        if (res <= 0) res = shs_internal::lib_resolve_resident_blocks(ctx->device, plan.prog, plan.wide, plan.sky);
        resolve_grid = std::max(1, std::min(plan.fp.n_owned_rt, res));
    }
    if (size_lib_pass(ctx, w, plan, shs_plan::build_draw_table(w.last_draws, plan.setup_blocks), raster_grid, ps)) return SHS_ERR_HIP;
    LibBuffers fb;
    bind_lib_pass(ctx, w, plan, shadow, *order, fb);
    return launch_lib_pass(ctx, w, plan, fb, shadow, raster_grid, resolve_grid, ps);
}

namespace {

uint32_t next_pow2(uint64_t v) {
    uint32_t p = 1;
    while (p < v && p < (1u << 30)) p <<= 1;
    return p;
}

// Read one pass's counters and statistics; grows what overflowed and returns true then.
int check_pass(shs_ctx *ctx, Work &w, bool &grew) {
    grew = false;
    if (!w.need_check) return SHS_OK;
    uint32_t *c = ctx->h_lib_counters;
    HIP_TRY(ctx, hipMemcpy(c, w.counters.p + w.last_parity * shs_dev::LC_N, shs_dev::LC_N * sizeof(uint32_t),
                           hipMemcpyDeviceToHost));
    std::vector<uint2> bs(w.last_setup_blocks), rs(w.last_raster_grid);
    HIP_TRY(ctx, hipMemcpy(bs.data(), w.blk_stat.p, bs.size() * sizeof(uint2), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(rs.data(), w.rstat.p, rs.size() * sizeof(uint2), hipMemcpyDeviceToHost));
    w.st_clip = w.st_raster = w.st_covered = w.st_maxbin = 0;
    for (const uint2 &b : bs) { w.st_clip += b.x; w.st_raster += b.y; }
    for (const uint2 &r : rs) { w.st_covered += r.x; w.st_maxbin = std::max<uint64_t>(w.st_maxbin, r.y); }
    if (&w == &ctx->lib_cam) w.st_covered = c[shs_dev::LC_COVERED];   // counted by k_lib_resolve
    w.st_spill = c[shs_dev::LC_SPILL];
    w.st_extra = c[shs_dev::LC_EXTRA];
    if (w.st_maxbin > w.bin_cap) w.bin_cap = next_pow2(std::min<uint64_t>(w.st_maxbin, 1u << 24));
    w.st_checked = true;
    const uint32_t ov = c[shs_dev::LC_OVERFLOW];
    if (ov & shs_dev::LOV_SPILL) {
        const size_t need = c[shs_dev::LC_SPILL];
        release(w.spill);
        if (ensure(ctx, w.spill, need + need / 4 + 1024)) return SHS_ERR_HIP;
        grew = true;
    }
    if (ov & shs_dev::LOV_EXTRA) {
        w.extra_cap = (uint32_t)std::min<uint64_t>((uint64_t)c[shs_dev::LC_EXTRA] + c[shs_dev::LC_EXTRA] / 4 + 4096, 1u << 28);
        grew = true;
    }
    w.need_check = false;
    return SHS_OK;
}

}  // namespace

// Wait for the enqueued passes; a pass that overflowed a capacity is re-issued (and a camera pass
// that sampled a re-issued shadow map with it).
int shs_lib_host::lib_finish(shs_ctx *ctx) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int attempt = 0; attempt < 6; ++attempt) {
        bool g_sh = false, g_cam = false;
        if (check_pass(ctx, ctx->lib_shadow, g_sh) || check_pass(ctx, ctx->lib_cam, g_cam)) return SHS_ERR_HIP;
        if (!g_sh && !g_cam) return SHS_OK;
        if (g_sh && enqueue_pass(ctx, ctx->lib_shadow, true)) return SHS_ERR_HIP;
        if ((g_cam || (g_sh && ctx->cam_after_shadow)) && ctx->lib_cam.done) {
            if (enqueue_pass(ctx, ctx->lib_cam, false)) return SHS_ERR_HIP;
            if (ctx->have_ldr && shs_tonemap_reissue(ctx)) return SHS_ERR_HIP;
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->err = "capacity overflow persisted";
    return SHS_ERR_OVERFLOW;
}

int shs_lib_host::check_superseded(shs_ctx *ctx, Work &w) {
    if (!w.need_check || !w.ov_valid) return SHS_OK;
    HIP_TRY(ctx, hipEventSynchronize(w.ov_after));
    return *w.h_ov ? lib_finish(ctx) : SHS_OK;
}

int shs_lib_host::check_lib_mesh(shs_ctx *ctx, int32_t id) {
    if (id < 0 || id >= (int)ctx->meshes.size() || !ctx->meshes[id].live || !ctx->meshes[id].lib) {
        ctx->err = "bad mesh id (not a library mesh)";
        return SHS_ERR_INVALID;
    }
    return SHS_OK;
}

const shs_ctx::OrderEntry *shs_lib_host::order_find(const std::vector<shs_ctx::OrderEntry> &cache, const uint64_t (&key)[4]) {
    for (const auto &e : cache)
        if (std::memcmp(e.key, key, sizeof key) == 0) return &e;
    return nullptr;
}

int shs_lib_host::order_insert(shs_ctx *ctx, std::vector<shs_ctx::OrderEntry> &cache, const uint64_t (&key)[4],
                               const std::vector<int32_t> &v, int n_owned, const shs_ctx::OrderEntry *&out) {
    if (cache.size() >= ORDER_CACHE) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->setup_stream));
        for (auto &e : cache) (void)hipFree(e.dev);
        cache.clear();
    }
    shs_ctx::OrderEntry e;
    std::memcpy(e.key, key, sizeof key);
    e.n = (int)v.size();
    e.n_owned = n_owned;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&e.dev), std::max<size_t>(v.size(), 1) * sizeof(int32_t)));
    if (!v.empty()) HIP_TRY(ctx, hipMemcpy(e.dev, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    cache.push_back(e);
    out = &cache.back();
    return SHS_OK;
}

int shs_lib_ensure_final(shs_ctx *ctx) {
    const int rc = check_superseded(ctx, ctx->lib_shadow);
    return rc ? rc : check_superseded(ctx, ctx->lib_cam);
}

void shs_lib_release(shs_ctx *ctx) {
    release_work(ctx->lib_cam);
    release_work(ctx->lib_shadow);
    for (auto *cache : {&ctx->rt_orders, &ctx->cull_orders}) {
        for (auto &e : *cache) (void)hipFree(e.dev);
        cache->clear();
    }
    for (auto &t : ctx->textures)
        if (t.texels) (void)hipFree(t.texels);
    ctx->textures.clear();
    release(ctx->srgb_lut);
    release(ctx->lib_hdr); release(ctx->lib_keys); release(ctx->lib_blkcov); ctx->blkcov_zero_at = nullptr; release(ctx->tm_thr_dev); ctx->tm_thr_dev_gamma = -1.0f; release(ctx->lib_depth); release(ctx->lib_motion); release(ctx->shadow_map);
    release(ctx->lights); release(ctx->tlights); release(ctx->depth_ranges);
    release(ctx->list_counts); release(ctx->list_indices); release(ctx->lib_timeline); release(ctx->lib_stimeline);
    release(ctx->lib_ldr); release(ctx->lib_present); release(ctx->lib_mb); release(ctx->lib_mb_present); release(ctx->lib_shaft_mask);
    release(ctx->lb_lights); release(ctx->lb_ndc); release(ctx->lb_counts); release(ctx->lb_indices);
    release(ctx->occ_depth); release(ctx->occ_visible); release(ctx->occ_flags); release(ctx->occ_objs); release(ctx->occ_rects); release(ctx->occ_tris);
    release(ctx->dd_objs); release(ctx->dd_tris); release(ctx->dd_depth0); release(ctx->dd_depth); release(ctx->dd_lit_b);
    release(ctx->dd_rgba); release(ctx->dd_keys); release(ctx->dd_big);
    release(ctx->cp_a); release(ctx->cp_b); release(ctx->cp_src); release(ctx->cp_depth); release(ctx->cp_vel); release(ctx->cp_focus); release(ctx->cp_map); release(ctx->cp_pq);
    release(ctx->fx_a); release(ctx->fx_b); release(ctx->fx_c); release(ctx->fx_in); release(ctx->fx_out); release(ctx->fx_depth); release(ctx->fx_vel); release(ctx->fx_spec); release(ctx->fx_pong);
    if (ctx->h_lib_counters) (void)hipHostFree(ctx->h_lib_counters);
    ctx->h_lib_counters = nullptr;
}

// shs_render_pbr_forward's checks, in order: the first that fails sets ctx->err.
static int validate_pbr_forward(shs_ctx *ctx, const shs_lib_frame &f, const shs_lib_draw *draws, int32_t n_draws) {
    if (f.width <= 0 || f.height <= 0 || f.width > 16384 || f.height > 16384) { ctx->err = "bad frame size"; return SHS_ERR_INVALID; }
    if (f.shard_count <= 0 || f.shard_rank < 0 || f.shard_rank >= f.shard_count) { ctx->err = "bad shard"; return SHS_ERR_INVALID; }
    for (int i = 0; i < n_draws; ++i) {
        if (check_lib_mesh(ctx, draws[i].mesh_id)) return SHS_ERR_INVALID;
        if (draws[i].program < SHS_PROGRAM_PBR_MR || draws[i].program > SHS_PROGRAM_FORWARD_PLUS_TYPED) { ctx->err = "bad program"; return SHS_ERR_INVALID; }
        if ((draws[i].program == SHS_PROGRAM_FORWARD_PLUS || draws[i].program == SHS_PROGRAM_FORWARD_PLUS_TYPED) &&
            (!ctx->have_cull || ctx->cull.W != f.width || ctx->cull.H != f.height)) {
            ctx->err = "Forward+ draw needs shs_light_cull for this frame size";
            return SHS_ERR_INVALID;
        }
        if (draws[i].program == SHS_PROGRAM_FORWARD_PLUS_TYPED && !(ctx->lights_typed && ctx->cull_typed)) {
            ctx->err = "typed Forward+ draw needs shs_lights_upload_typed and a shs_light_cull after it";
            return SHS_ERR_INVALID;
        }
        if (draws[i].cull_mode < SHS_CULL_NONE || draws[i].cull_mode > SHS_CULL_FRONT) { ctx->err = "bad cull mode"; return SHS_ERR_INVALID; }
        if (draws[i].shadow && !ctx->have_shadow) { ctx->err = "draw samples a shadow map but none was rendered"; return SHS_ERR_INVALID; }
        const int32_t tx = draws[i].base_color_tex;
        if (tx < 0 || tx > (int32_t)ctx->textures.size() || (tx > 0 && !ctx->textures[(size_t)tx - 1].live)) {
            ctx->err = "bad base_color_tex (not a live texture id)";
            return SHS_ERR_INVALID;
        }
    }
    return SHS_OK;
}

// The camera pass's targets of a frame: HDR, winners, block flags, (SHS_LIB_DEPTH_MOTION) depth and motion.
static int ensure_camera_targets(shs_ctx *ctx, const shs_lib_frame &f) {
    const size_t npx = (size_t)f.width * f.height;
    if (ensure(ctx, ctx->lib_hdr, npx) || ensure(ctx, ctx->lib_keys, npx)) return SHS_ERR_HIP;
    const size_t n_blk = (size_t)((f.width + 31) / 32) * ((f.height + 7) / 8) * 4;   // 16x4 blocks
    if (ensure(ctx, ctx->lib_blkcov, n_blk)) return SHS_ERR_HIP;
    // the block flags start at zero (then every resolve leaves them so); rare: a sync memset
    const uint64_t bk = (uint64_t)(uint32_t)f.width | ((uint64_t)(uint32_t)f.height << 32);
    if (ctx->blkcov_zero_at != ctx->lib_blkcov.p || ctx->blkcov_zero_cap != ctx->lib_blkcov.cap || ctx->blkcov_zero_key != bk) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->setup_stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->setup_stream));
        HIP_TRY(ctx, hipMemset(ctx->lib_blkcov.p, 0, ctx->lib_blkcov.cap * sizeof(uint32_t)));
        ctx->blkcov_zero_at = ctx->lib_blkcov.p;
        ctx->blkcov_zero_cap = ctx->lib_blkcov.cap;
        ctx->blkcov_zero_key = bk;
    }
    if ((f.flags & SHS_LIB_DEPTH_MOTION) && (ensure(ctx, ctx->lib_depth, npx) || ensure(ctx, ctx->lib_motion, npx))) return SHS_ERR_HIP;
    return SHS_OK;
}

// The camera pass as recorded (Work::last_fp): the frame, this rank's share, the context's sky, shadow
// map size and light lists.  The plan fills the rest.
static int camera_frame_params(shs_ctx *ctx, const shs_lib_frame &f, bool regions, LibFrameParams &fp) {
    std::memset(&fp, 0, sizeof fp);
    fp.W = f.width; fp.H = f.height;
    fp.rank = f.shard_rank; fp.count = f.shard_count;
    if (regions) {   // this rank's rectangle of the balanced layout (the pass's light cull used the same)
        if (shs_regions_next(ctx, f.shard_count, f.width, f.height)) return SHS_ERR_HIP;
        fp.reg = ctx->reg_next[(size_t)f.shard_rank];
    }
    fp.flags = (f.flags & SHS_LIB_BG_GRADIENT) ? shs_dev::LF_GRADIENT : 0u;
    if (f.flags & SHS_LIB_DEPTH_MOTION) {
        fp.flags |= shs_dev::LF_DEPTH | shs_dev::LF_MOTION;
        if (f.zf > f.zn + 1e-6f) fp.flags |= shs_dev::LF_LINZ;   // rasterizer.hpp:354
    }
    fp.zn = f.zn; fp.zf = f.zf; fp.zspan = f.zf - f.zn;
    for (int i = 0; i < 4; ++i) fp.clear[i] = f.clear_hdr[i];
    fp.sky = ctx->sky;   // kept in wk.last_fp: a re-issue replays the sky this pass was enqueued with
    fp.sm_w = ctx->shadow_w; fp.sm_h = ctx->shadow_h;
    if (ctx->have_cull) {
        const shs_dev::LightCullParams &c = ctx->cull;
        fp.lt_size = c.tile_size; fp.lt_tx = c.tiles_x; fp.lt_ty = c.tiles_y; fp.lt_maxp = c.max_per_tile;
        fp.lt_mode = c.mode; fp.lt_zs = c.z_slices; fp.n_lights = c.n_lights;
        fp.lt_view_z[0] = c.view[2]; fp.lt_view_z[1] = c.view[6]; fp.lt_view_z[2] = c.view[10]; fp.lt_view_z[3] = c.view[14];
        fp.lt_zn = c.zn; fp.lt_zf = c.zf;
    }
    return SHS_OK;
}

extern "C" {

int shs_render_pbr_forward(shs_ctx *ctx, const shs_lib_frame *frame, const shs_lib_draw *draws, int32_t n_draws) {
    if (!ctx || !frame || n_draws < 0 || (n_draws > 0 && !draws)) return SHS_ERR_INVALID;
    const shs_lib_frame &f = *frame;
    if (validate_pbr_forward(ctx, f, draws, n_draws)) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    if (!ctx->h_lib_counters && hipHostMalloc(reinterpret_cast<void **>(&ctx->h_lib_counters), shs_dev::LC_N * sizeof(uint32_t)) != hipSuccess)
        return SHS_ERR_HIP;
    {   // the pending camera pass is checked before this one rewrites its targets
        const int rc = check_superseded(ctx, ctx->lib_cam);
        if (rc) return rc;
    }
    if (ensure_camera_targets(ctx, f)) return SHS_ERR_HIP;
    Work &wk = ctx->lib_cam;
    wk.last_draws.resize(n_draws);
    int32_t base = 0;
    for (int i = 0; i < n_draws; ++i) {
        const Mesh &m = ctx->meshes[draws[i].mesh_id];
        build_lib_draw(draws[i], m, base, wk.last_draws[i]);
        bind_texture(ctx, draws[i].base_color_tex, wk.last_draws[i]);
        base += m.n_tris;
    }
    const bool regions = f.shard_count > 1 && ctx->shard_layout == SHS_SHARD_REGIONS;
    if (camera_frame_params(ctx, f, regions, wk.last_fp)) return SHS_ERR_HIP;
    {
        const int rc = shadow_for_camera(ctx, f, draws, n_draws, wk.last_fp.reg);
        if (rc) return rc;
    }
    ctx->lib_frame = f;
    // The camera pass runs on the context's stream after its shadow pass (round 6): with three frames in
    // flight the frames overlap each other, and a context with one busy stream keeps the process's 4
    // hardware queues to one stream per frame -- on the side stream beside the shadow pass, C5's strong
    // leg after the C4 leg read 0.394-0.405 against 0.370-0.371 ms per frame, --config c5 unchanged
    // (profiles/r06_c5_one_stream_ab.txt).  (SHS_EXP_CAM_SIDE_STREAM: the side stream, timing only.)
#ifdef SHS_EXP_CAM_SIDE_STREAM
    ctx->cam_after_shadow = ctx->have_shadow;
#else
    ctx->cam_after_shadow = false;
#endif
    wk.tm_fused = ctx->tm_fuse;
    wk.tm_desc = ctx->tm_fuse_desc;
    const int rc = enqueue_pass(ctx, wk, false);
    if (rc) return rc;
    if (regions) {   // the layout of this pass (tonemap, gather); the next pass balances anew
        ctx->reg_last = ctx->reg_next;
        ctx->reg_last_count = f.shard_count;
        ctx->reg_next_fresh = false;
    } else {
        ctx->reg_last.clear();
        ctx->reg_last_count = 0;
    }
    ctx->have_lib_frame = true;
    // a new camera pass: a tonemap (and motion blur) must follow it again, unless it ran fused
    ctx->have_ldr = wk.tm_fused;
    if (wk.tm_fused) ctx->tm_desc = wk.tm_desc;
    ctx->have_ls = false;
    ctx->have_mb = false;
    return SHS_OK;
}

int shs_resolve_lib(shs_ctx *ctx, float *hdr, float *depth, float *motion) {
    if (!ctx) return SHS_ERR_INVALID;
    if (!ctx->have_lib_frame) { ctx->err = "no library frame rendered"; return SHS_ERR_INVALID; }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    int rc = lib_finish(ctx);
    if (rc) return rc;
    const size_t npx = (size_t)ctx->lib_frame.width * ctx->lib_frame.height;
    const bool dm = (ctx->lib_frame.flags & SHS_LIB_DEPTH_MOTION) != 0;
    if ((depth || motion) && !dm) { ctx->err = "frame has no depth_motion target"; return SHS_ERR_INVALID; }
    if (hdr) HIP_TRY(ctx, hipMemcpy(hdr, ctx->lib_hdr.p, npx * sizeof(float4), hipMemcpyDeviceToHost));
    if (depth) HIP_TRY(ctx, hipMemcpy(depth, ctx->lib_depth.p, npx * sizeof(float), hipMemcpyDeviceToHost));
    if (motion) HIP_TRY(ctx, hipMemcpy(motion, ctx->lib_motion.p, npx * sizeof(float2), hipMemcpyDeviceToHost));
    return SHS_OK;
}

int shs_lib_debug_setup_timeline(shs_ctx *ctx, uint64_t *out, int64_t capacity, int64_t *n_out) {
    if (!ctx || !n_out) return SHS_ERR_INVALID;
    if (!ctx->want_timeline || !ctx->lib_stimeline.p || ctx->lib_cam.last_setup_blocks <= 0) {
        ctx->err = "timeline not enabled or no camera pass yet";
        return SHS_ERR_INVALID;
    }
    const int64_t n = (int64_t)ctx->lib_cam.last_setup_blocks * shs_dev::STL_STRIDE;
    *n_out = n;
    if (!out) return SHS_OK;
    if (capacity < n) { ctx->err = "capacity too small"; return SHS_ERR_INVALID; }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->lib_stimeline.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SHS_OK;
}

int shs_lib_debug_timeline(shs_ctx *ctx, uint64_t *out, int64_t capacity, int64_t *n_out) {
    if (!ctx || !n_out) return SHS_ERR_INVALID;
    const Work &tw = ctx->timeline_shadow ? ctx->lib_shadow : ctx->lib_cam;
    if (!ctx->want_timeline || !ctx->lib_timeline.p || tw.last_raster_grid <= 0) {
        ctx->err = "timeline not enabled or no such pass yet";
        return SHS_ERR_INVALID;
    }
    const int64_t n = (int64_t)tw.last_raster_grid * shs_dev::LTL_STRIDE;
    *n_out = n;
    if (!out) return SHS_OK;
    if (capacity < n) { ctx->err = "capacity too small"; return SHS_ERR_INVALID; }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->lib_timeline.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SHS_OK;
}

int shs_get_lib_stats(shs_ctx *ctx, shs_lib_stats *st) {
    if (!ctx || !st || !ctx->have_lib_frame) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    int rc = lib_finish(ctx);
    if (rc) return rc;
    const Work &w = ctx->lib_cam;
    st->tri_input = (uint64_t)w.last_n_tris;
    st->tri_after_clip = w.st_clip;
    st->tri_raster = w.st_raster;
    st->covered_pixels = w.st_covered;
    st->max_tile_bin = w.st_maxbin;
    st->spilled = w.st_spill;
    st->clipped_extra = w.st_extra;
    return SHS_OK;
}

int shs_lib_device_targets(shs_ctx *ctx, void **hdr_dev, void **depth_dev, void **motion_dev) {
    if (!ctx || !ctx->have_lib_frame) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const int rc = lib_finish(ctx);   // the pass is final (re-issued on overflow) before it is handed out
    if (rc) return rc;
    if (hdr_dev) *hdr_dev = ctx->lib_hdr.p;
    if (depth_dev) *depth_dev = ctx->lib_depth.p;
    if (motion_dev) *motion_dev = ctx->lib_motion.p;
    return SHS_OK;
}

int shs_lib_timing_reset(shs_ctx *ctx) {
    if (!ctx) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (Work *w : {&ctx->lib_shadow, &ctx->lib_cam}) {
        if (harvest_all(ctx, *w)) return SHS_ERR_HIP;
        w->acc_ms[0] = w->acc_ms[1] = 0.0;
        w->acc_n = 0;
    }
    return SHS_OK;
}

int shs_lib_timing_read(shs_ctx *ctx, double sum_ms4[4], int64_t n_passes2[2]) {
    if (!ctx || !sum_ms4 || !n_passes2) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (harvest_all(ctx, ctx->lib_shadow) || harvest_all(ctx, ctx->lib_cam)) return SHS_ERR_HIP;
    sum_ms4[0] = ctx->lib_shadow.acc_ms[0]; sum_ms4[1] = ctx->lib_shadow.acc_ms[1];
    sum_ms4[2] = ctx->lib_cam.acc_ms[0]; sum_ms4[3] = ctx->lib_cam.acc_ms[1];
    n_passes2[0] = ctx->lib_shadow.acc_n;
    n_passes2[1] = ctx->lib_cam.acc_n;
    return SHS_OK;
}

}  // extern "C"
