// shs_abi_tiles.cpp -- the tile pack / unpack ABI of libshs_gpu.so (include/shs_gpu.h): a shard's owned
// 32x32 tiles of a legacy or library target to and from a packed device buffer (shs_tiles.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/shs_gpu.h"
#include "shs_ctx.hpp"
#include "shs_tiles_internal.hpp"

static int tile_params(shs_ctx *ctx, int target, int32_t rank, int32_t count, shs_dev::TileCopyParams &p) {
    std::memset(&p, 0, sizeof p);
    if (count <= 0 || rank < 0 || rank >= count) { ctx->err = "bad shard"; return SHS_ERR_INVALID; }
    p.rank = rank;
    p.count = count;
    // a region-sharded library frame: rank's rectangle of the last camera pass's layout
    if ((target == SHS_TARGET_LIB || target == SHS_TARGET_LIB_PRESENT) && count > 1 && ctx->reg_last_count == count)
        p.reg = ctx->reg_last[(size_t)rank];
    if (target == SHS_TARGET_LEGACY) {
        if (!ctx->have_frame) { ctx->err = "no legacy frame rendered"; return SHS_ERR_INVALID; }
        p.W = ctx->frame.width; p.H = ctx->frame.height;
        p.color_words = 1; p.color_flip = 1;
        p.color = reinterpret_cast<uint32_t *>(ctx->color.p);
        p.depth = reinterpret_cast<uint32_t *>(ctx->depth.p);
    } else if (target == SHS_TARGET_PRESENT) {
        // the legacy frame's SDL staging: screen rows, the legacy tiles' own row order
        if (!ctx->have_frame || !(ctx->frame.flags & SHS_FRAME_PRESENT)) { ctx->err = "no legacy present staging"; return SHS_ERR_INVALID; }
        p.W = ctx->frame.width; p.H = ctx->frame.height;
        p.color_words = 1; p.color_flip = 0;
        p.color = ctx->present.p;
    } else if (target == SHS_TARGET_LIB_PRESENT) {
        // the last tonemap's present staging: rows top-down, library tiles count rows y up
        if (!ctx->have_ldr || !(ctx->tm_desc.flags & SHS_TONEMAP_PRESENT)) { ctx->err = "no tonemap present staging"; return SHS_ERR_INVALID; }
        p.W = ctx->lib_frame.width; p.H = ctx->lib_frame.height;
        p.color_words = 1; p.color_flip = 1;
        p.color = ctx->lib_present.p;
    } else if (target == SHS_TARGET_LIB) {
        if (!ctx->have_lib_frame) { ctx->err = "no library frame rendered"; return SHS_ERR_INVALID; }
        p.W = ctx->lib_frame.width; p.H = ctx->lib_frame.height;
        p.color_words = 4; p.color_flip = 0;
        p.color = reinterpret_cast<uint32_t *>(ctx->lib_hdr.p);
        if (ctx->lib_frame.flags & SHS_LIB_DEPTH_MOTION) {
            p.depth = reinterpret_cast<uint32_t *>(ctx->lib_depth.p);
            p.motion = reinterpret_cast<uint32_t *>(ctx->lib_motion.p);
        }
    } else {
        ctx->err = "bad target";
        return SHS_ERR_INVALID;
    }
    p.words = p.color_words + (p.depth ? 1 : 0) + (p.motion ? 2 : 0);
    return SHS_OK;
}

// A frame whose capacity overflowed is re-issued before its tiles leave the rank or peers' tiles land in
// it (legacy: the batch, a pipelined batch's pending raster included -- it clears the whole frame;
// library: the pass chain, tonemap included).  Only its setup is waited for: the overflow word is final
// then, and the copy is stream-ordered after the (possibly re-issued) frame.
static int final_before_copy(shs_ctx *ctx, int target) {
    return (target == SHS_TARGET_LEGACY || target == SHS_TARGET_PRESENT) ? shs_legacy_ensure_final(ctx)
                                                                        : shs_lib_ensure_final(ctx);
}

extern "C" {

int shs_tiles_rank_words(shs_ctx *ctx, int target, int32_t rank, int32_t count, int64_t *words_out) {
    if (!ctx || !words_out) return SHS_ERR_INVALID;
    shs_dev::TileCopyParams p;
    if (tile_params(ctx, target, rank, count, p)) return SHS_ERR_INVALID;
    const int n_tiles = ((p.W + 31) / 32) * ((p.H + 31) / 32);
    *words_out = (int64_t)shs_dev::shard_n_owned(rank, count, p.reg, n_tiles) * 32 * 32 * p.words;
    return SHS_OK;
}

int shs_tiles_packed_words(shs_ctx *ctx, int target, int32_t count, int64_t *words_out) {
    if (!ctx || !words_out) return SHS_ERR_INVALID;
    int64_t most = 0;
    for (int32_t r = 0; r < std::max(count, 1); ++r) {
        int64_t w = 0;
        if (shs_tiles_rank_words(ctx, target, r, count, &w)) return SHS_ERR_INVALID;
        most = std::max(most, w);
    }
    *words_out = most;
    return SHS_OK;
}

int shs_tiles_pack(shs_ctx *ctx, int target, int32_t rank, int32_t count, void *dst_dev) {
    if (!ctx || !dst_dev) return SHS_ERR_INVALID;
    shs_dev::TileCopyParams p;
    if (tile_params(ctx, target, rank, count, p)) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const int rc = final_before_copy(ctx, target);
    if (rc) return rc;
    HIP_TRY(ctx, shs_internal::launch_tiles_copy(p, true, dst_dev, ctx->stream));
    return SHS_OK;
}

int shs_tiles_unpack(shs_ctx *ctx, int target, int32_t rank, int32_t count, const void *src_dev) {
    if (!ctx || !src_dev) return SHS_ERR_INVALID;
    shs_dev::TileCopyParams p;
    if (tile_params(ctx, target, rank, count, p)) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const int rc = final_before_copy(ctx, target);
    if (rc) return rc;
    // tiles land in the legacy planes from outside the rasters: the next legacy batch clears fully
    if (target == SHS_TARGET_LEGACY || target == SHS_TARGET_PRESENT) ctx->planes_known = false;
    HIP_TRY(ctx, shs_internal::launch_tiles_copy(p, false, const_cast<void *>(src_dev), ctx->stream));
    return SHS_OK;
}

int shs_tiles_unpack_ranks(shs_ctx *ctx, int target, int32_t count, const void *const *src_dev) {
    if (!ctx || !src_dev || count <= 0) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    {
        const int rc = final_before_copy(ctx, target);
        if (rc) return rc;
    }
    if (target == SHS_TARGET_LEGACY || target == SHS_TARGET_PRESENT) ctx->planes_known = false;   // as shs_tiles_unpack
    shs_dev::TileUnpackMulti m;
    std::memset(&m, 0, sizeof m);
    for (int32_t r = 0; r < count; ++r) {
        if (!src_dev[r]) continue;
        shs_dev::TileCopyParams p;
        if (tile_params(ctx, target, r, count, p)) return SHS_ERR_INVALID;
        const int n_tiles = ((p.W + shs_dev::TILE - 1) / shs_dev::TILE) * ((p.H + shs_dev::TILE - 1) / shs_dev::TILE);
        const int owned = shs_dev::shard_n_owned(p.rank, p.count, p.reg, n_tiles);
        if (owned <= 0) continue;
        if (m.n == shs_dev::UNPACK_PEERS) {   // a launch per UNPACK_PEERS peers
            HIP_TRY(ctx, shs_internal::launch_tiles_unpack_multi(m, ctx->stream));
            std::memset(&m, 0, sizeof m);
        }
        m.p = p;
        m.rank[m.n] = r;
        m.reg[m.n] = p.reg;
        m.src[m.n] = static_cast<const uint32_t *>(src_dev[r]);
        m.first[m.n + 1] = m.first[m.n] + owned;
        ++m.n;
    }
    HIP_TRY(ctx, shs_internal::launch_tiles_unpack_multi(m, ctx->stream));
    return SHS_OK;
}

}  // extern "C"
