// shs_abi_light_cull.cpp -- the Forward+ light lists of the library path (include/shs_gpu.h): the light
// set's upload, the tile / cluster cull (shs_light.hip) and the lists' readback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/shs_gpu.h"
#include "shs_ctx.hpp"
#include "shs_lib_host.hpp"
#include "shs_light_internal.hpp"

using namespace shs_lib_host;

// Tile-sharded cull: the rank's lists first, then the rest (the cached table of a shard layout).
static std::vector<int32_t> owned_lists_first(const shs_dev::LightCullParams &p, int &n_owned) {
    std::vector<int32_t> v, rest;
    const uint32_t per_slice = p.tiles_x * p.tiles_y;
    for (uint32_t l = 0; l < p.n_lists; ++l) {
        const uint32_t rem = l % per_slice;
        (shs_internal::light_list_owned(p, rem % p.tiles_x, rem / p.tiles_x) ? v : rest).push_back((int32_t)l);
    }
    n_owned = (int)v.size();
    v.insert(v.end(), rest.begin(), rest.end());
    return v;
}

extern "C" {

int shs_lights_upload(shs_ctx *ctx, const shs_culling_light *lights, int32_t n) {
    static_assert(sizeof(shs_culling_light) == sizeof(shs_dev::CullLight), "CullingLightGPU layout");
    if (!ctx || n < 0 || (n > 0 && !lights)) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    if (ensure(ctx, ctx->lights, (size_t)std::max(n, 1))) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the previous set may still be read
    if (n > 0) HIP_TRY(ctx, hipMemcpy(ctx->lights.p, lights, (size_t)n * sizeof(shs_dev::CullLight), hipMemcpyHostToDevice));
    ctx->n_lights = n;
    ctx->lights_typed = ctx->cull_typed = false;   // (shs_lights_upload_typed sets the first after this call)
    return SHS_OK;
}

int shs_light_cull(shs_ctx *ctx, const shs_light_cull_desc *d) {
    if (!ctx || !d) return SHS_ERR_INVALID;
    if (d->width <= 0 || d->height <= 0 || d->tile_size == 0 || d->max_per_tile == 0 || d->mode > 3u ||
        (d->mode == 3u && d->z_slices == 0) || d->shard_count <= 0 || d->shard_rank < 0 || d->shard_rank >= d->shard_count) {
        ctx->err = "bad light cull description";
        return SHS_ERR_INVALID;
    }
    if (d->mode == 2u && (!ctx->have_lib_frame || !(ctx->lib_frame.flags & SHS_LIB_DEPTH_MOTION) ||
                          ctx->lib_frame.width != d->width || ctx->lib_frame.height != d->height)) {
        ctx->err = "tiled-depth culling needs a library frame with a depth target of the same size";
        return SHS_ERR_INVALID;
    }
    if (d->mode == 2u && d->shard_count > 1 && ctx->shard_layout == SHS_SHARD_REGIONS) {
        // the depth ranges come from the previous camera pass's depth, which a region rank holds only for
        // its previous rectangle; rectangles move between passes, so a newly owned tile would read stale
        // depth.  Interleaved ownership is static and keeps the depth of every owned tile.
        ctx->err = "tiled-depth culling needs the interleaved shard layout (region rectangles move between passes)";
        return SHS_ERR_INVALID;
    }
    if (d->mode == 2u && d->shard_count > 1 && (32u % d->tile_size) == 0u && ((uint32_t)d->height % 32u) % d->tile_size != 0u) {
        // light tiles count rows top-down, bin tiles bottom-up: at this height a light tile straddles two
        // bin rows, i.e. two ranks' pixels, and its depth range would read the other rank's stale depth
        ctx->err = "sharded tiled-depth culling needs height % 32 to be a multiple of the light tile size";
        return SHS_ERR_INVALID;
    }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    if (d->mode == 2u) {   // the depth it reduces must be final: an overflowed camera pass is re-issued first
        const int rc = check_superseded(ctx, ctx->lib_cam);
        if (rc) return rc;
    }
    shs_dev::LightCullParams p;
    std::memset(&p, 0, sizeof p);
    p.W = d->width; p.H = d->height;
    p.tile_size = d->tile_size; p.max_per_tile = d->max_per_tile; p.mode = d->mode;
    p.z_slices = std::max(d->z_slices, 1u);
    p.tiles_x = (d->width + d->tile_size - 1) / d->tile_size;
    p.tiles_y = (d->height + d->tile_size - 1) / d->tile_size;
    p.n_lists = p.tiles_x * p.tiles_y * (d->mode == 3u ? p.z_slices : 1u);
    p.n_lights = (uint32_t)ctx->n_lights;
    p.zn = d->zn; p.zf = d->zf;
    p.depth_linear = d->depth_linear;
    p.rank = d->shard_rank; p.count = d->shard_count;
    if (p.count > 1 && ctx->shard_layout == SHS_SHARD_REGIONS) {   // the upcoming camera pass's rectangle
        if (shs_regions_next(ctx, p.count, p.W, p.H)) return SHS_ERR_HIP;
        p.reg = ctx->reg_next[(size_t)p.rank];
    }
    std::memcpy(p.view, d->view, sizeof p.view);
    std::memcpy(p.proj, d->proj, sizeof p.proj);
    if (ensure(ctx, ctx->depth_ranges, (size_t)p.tiles_x * p.tiles_y) || ensure(ctx, ctx->list_counts, p.n_lists) ||
        ensure(ctx, ctx->list_indices, (size_t)p.n_lists * p.max_per_tile) || ensure(ctx, ctx->lights, 1))
        return SHS_ERR_HIP;
    const uint32_t *work = nullptr;
    uint32_t n_work = p.n_lists;
    if (p.count > 1 && (32u % p.tile_size) == 0u) {   // tile-sharded: this rank's lists first (cached table)
        const uint64_t key[4] = {(uint64_t)(uint32_t)p.W | ((uint64_t)(uint32_t)p.H << 32),
                                 (uint64_t)p.tile_size | ((uint64_t)p.n_lists << 32),
                                 (uint64_t)(uint32_t)p.rank | ((uint64_t)(uint32_t)p.count << 32),
                                 p.reg.on ? region_key(p.reg) ^ (1ull << 63) : 0ull};
        const shs_ctx::OrderEntry *e = order_find(ctx->cull_orders, key);
        if (!e) {
            int n_owned = 0;
            const std::vector<int32_t> v = owned_lists_first(p, n_owned);
            if (order_insert(ctx, ctx->cull_orders, key, v, n_owned, e)) return SHS_ERR_HIP;
        }
        work = reinterpret_cast<const uint32_t *>(e->dev);
        n_work = (uint32_t)e->n_owned;
    }
    HIP_TRY(ctx, shs_internal::launch_light_cull(p, ctx->lights.p, ctx->lib_depth.p, ctx->depth_ranges.p, work, n_work,
                                                 ctx->list_counts.p, ctx->list_indices.p, ctx->stream));
    ctx->cull = p;
    ctx->have_cull = true;
    ctx->cull_typed = ctx->lights_typed;
    return SHS_OK;
}

int shs_resolve_light_lists(shs_ctx *ctx, uint32_t *counts, uint32_t *indices, float *ranges) {
    if (!ctx) return SHS_ERR_INVALID;
    if (!ctx->have_cull) { ctx->err = "no light cull run"; return SHS_ERR_INVALID; }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const shs_dev::LightCullParams &p = ctx->cull;
    if (counts) HIP_TRY(ctx, hipMemcpy(counts, ctx->list_counts.p, p.n_lists * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (indices)
        HIP_TRY(ctx, hipMemcpy(indices, ctx->list_indices.p, (size_t)p.n_lists * p.max_per_tile * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (ranges)
        HIP_TRY(ctx, hipMemcpy(ranges, ctx->depth_ranges.p, (size_t)p.tiles_x * p.tiles_y * sizeof(float2), hipMemcpyDeviceToHost));
    return SHS_OK;
}

}  // extern "C"
