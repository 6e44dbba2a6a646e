// shs_lib_host.hpp -- the few library-path host helpers that several ABI translation units share
// (shs_abi_lib.cpp, shs_abi_shadow.cpp, shs_abi_mesh.cpp, shs_abi_sky.cpp, shs_abi_light_cull.cpp).
// Internal: none is exported.
#pragma once
#include <vector>

#include "shs_ctx.hpp"

#pragma GCC visibility push(hidden)
namespace shs_lib_host {

// Enqueue the pass that w.last_fp / w.last_draws describe; wait for the enqueued passes and re-issue what
// overflowed.  (shs_abi_lib.cpp)
int enqueue_pass(shs_ctx *ctx, shs_ctx::LibWork &w, bool shadow);
int lib_finish(shs_ctx *ctx);
// The shadow map a camera pass about to be enqueued samples is rendered where it reads it.  (shs_abi_shadow.cpp)
int shadow_for_camera(shs_ctx *ctx, const shs_lib_frame &f, const shs_lib_draw *draws, int32_t n_draws,
                      const shs_dev::ShardRegion &cam_reg);
// A pass about to be superseded (its workspace and targets rewritten) whose overflow word is set is
// finished first -- re-issued with grown capacities -- so no stream-ordered consumer of it (a tonemap,
// a copy, a gather queued behind it) sees an incomplete pass.  (shs_abi_lib.cpp)
int check_superseded(shs_ctx *ctx, shs_ctx::LibWork &w);
int check_lib_mesh(shs_ctx *ctx, int32_t id);   // SHS_ERR_INVALID (and ctx->err) unless id is a live library mesh
// srgb_to_linear_rgb's table, uploaded on first use (shs_abi_mesh.cpp)
int ensure_srgb_lut(shs_ctx *ctx);

inline uint64_t region_key(const shs_dev::ShardRegion &g) {
    return (uint64_t)(uint16_t)g.x0 | ((uint64_t)(uint16_t)g.y0 << 16) | ((uint64_t)(uint16_t)g.x1 << 32) |
           ((uint64_t)(uint16_t)g.y1 << 48);
}

// A device table (raster tile order, owned light lists) for a 4-word key, built and uploaded once into
// its own buffer: a synchronous copy into fresh memory waits for no stream, so a changed shard layout
// costs no pipeline drain.  Past ORDER_CACHE entries the cache is dropped (after the streams drain).
// order_find: the entry, or null (the caller builds the table and inserts it).  (shs_abi_lib.cpp)
constexpr size_t ORDER_CACHE = 48;
const shs_ctx::OrderEntry *order_find(const std::vector<shs_ctx::OrderEntry> &cache, const uint64_t (&key)[4]);
int order_insert(shs_ctx *ctx, std::vector<shs_ctx::OrderEntry> &cache, const uint64_t (&key)[4], const std::vector<int32_t> &v,
                 int n_owned, const shs_ctx::OrderEntry *&out);

}  // namespace shs_lib_host
#pragma GCC visibility pop
