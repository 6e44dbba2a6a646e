// shs_abi_mesh.cpp -- library-path resources of libshs_gpu.so (include/shs_gpu.h, "Library path"): MeshData
// upload with its spatial ordering, Texture2DData upload and release, the sRGB table their samplers read.
// Reference paths are relative to shs-renderer-lib/include/shs/.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/shs_gpu.h"
#include "shs_ctx.hpp"
#include "shs_lib_host.hpp"

// srgb_to_linear_rgb (builtin_shaders.hpp:25-31) and srgb_to_linear_approx (cubemap_sky.hpp:39-45) with the
// host's std::pow: the table the texture and sky samplers read
int shs_lib_host::ensure_srgb_lut(shs_ctx *ctx) {
    if (ctx->srgb_lut.p) return SHS_OK;
    float lut[256];
    for (int i = 0; i < 256; ++i) lut[i] = std::pow((float)i / 255.0f, 2.2f);
    if (ensure(ctx, ctx->srgb_lut, 256)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipMemcpy(ctx->srgb_lut.p, lut, sizeof lut, hipMemcpyHostToDevice));
    return SHS_OK;
}

// The stored order of a library mesh's triangles: MeshData indices sorted by the 30-bit Morton code of
// the centroid in the mesh's bounds (stable; triangles with an out-of-range index or a non-finite
// centroid last).  Empty when the mesh fits one chunk or the order is the identity.
static std::vector<uint32_t> spatial_order(const float *pos, int32_t n_verts, const uint32_t *idx, int32_t n_tris) {
    std::vector<uint32_t> order;
    if (n_tris <= 256) return order;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<float> cen((size_t)n_tris * 3);
    std::vector<uint8_t> ok((size_t)n_tris);
    for (int32_t t = 0; t < n_tris; ++t) {
        bool good = true;
        float c[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < 3; ++k) {
            const uint32_t v = idx ? idx[3 * (size_t)t + k] : (uint32_t)(3 * t + k);
            if (v >= (uint32_t)n_verts) { good = false; break; }
            for (int q = 0; q < 3; ++q) c[q] += pos[3 * (size_t)v + q];
        }
        for (int q = 0; q < 3 && good; ++q) good = std::isfinite(c[q]);
        ok[t] = good;
        for (int q = 0; q < 3; ++q) {
            cen[3 * (size_t)t + q] = c[q];
            if (good) { lo[q] = std::min(lo[q], c[q]); hi[q] = std::max(hi[q], c[q]); }
        }
    }
    auto spread = [](uint32_t x) {   // 10 bits -> every third bit
        x &= 0x3ffu;
        x = (x | (x << 16)) & 0x030000ffu;
        x = (x | (x << 8)) & 0x0300f00fu;
        x = (x | (x << 4)) & 0x030c30c3u;
        x = (x | (x << 2)) & 0x09249249u;
        return x;
    };
    std::vector<uint64_t> key((size_t)n_tris);
    for (int32_t t = 0; t < n_tris; ++t) {
        uint32_t code = 0xffffffffu;
        if (ok[t]) {
            code = 0u;
            for (int q = 0; q < 3; ++q) {
                const float ext = hi[q] - lo[q];
                const float u = ext > 0.0f ? (cen[3 * (size_t)t + q] - lo[q]) / ext : 0.0f;
                const uint32_t b = (uint32_t)std::min(1023.0f, std::max(0.0f, u * 1024.0f));
                code |= spread(b) << q;
            }
        }
        key[t] = ((uint64_t)code << 32) | (uint32_t)t;   // ties keep the MeshData order
    }
    std::sort(key.begin(), key.end());
    order.resize((size_t)n_tris);
    bool identity = true;
    for (int32_t p = 0; p < n_tris; ++p) {
        order[p] = (uint32_t)key[p];
        identity = identity && order[p] == (uint32_t)p;
    }
    if (identity) order.clear();
    return order;
}

// Model-space boxes (min, max) of the mesh's 256-triangle chunks (k_lib_setup's block bounds): out-of-range
// indices are skipped there
static std::vector<float4> chunk_boxes(const float *positions, int32_t n_verts, const uint32_t *indices, int32_t n_tris) {
    const int64_t n_chunks = ((int64_t)n_tris + 255) / 256;
    std::vector<float4> cb((size_t)n_chunks * 2);
    for (int64_t c = 0; c < n_chunks; ++c) {
        float mn[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}, mx[3] = {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f};
        const int64_t t1 = std::min<int64_t>(n_tris, (c + 1) * 256);
        for (int64_t t = c * 256; t < t1; ++t)
            for (int k = 0; k < 3; ++k) {
                const uint32_t v = indices ? indices[3 * t + k] : (uint32_t)(3 * t + k);
                if (v >= (uint32_t)n_verts) continue;
                for (int q = 0; q < 3; ++q) {
                    const float p = positions[3 * (size_t)v + q];
                    mn[q] = std::min(mn[q], p);
                    mx[q] = std::max(mx[q], p);
                }
            }
        cb[2 * c] = make_float4(mn[0], mn[1], mn[2], 0.0f);
        cb[2 * c + 1] = make_float4(mx[0], mx[1], mx[2], 0.0f);
    }
    return cb;
}

extern "C" {

int shs_mesh_upload(shs_ctx *ctx, const float *positions, int32_t n_verts, const float *normals, int32_t n_normals,
                    const float *uvs, int32_t n_uvs, const uint32_t *indices, int64_t n_indices, int32_t *mesh_id) {
    if (!ctx || !positions || n_verts <= 0 || !mesh_id || n_normals < 0 || n_uvs < 0 || n_indices < 0 ||
        (n_normals > 0 && !normals) || (n_uvs > 0 && !uvs) || (n_indices > 0 && !indices))
        return SHS_ERR_INVALID;
    const int64_t n_tris = indices ? n_indices / 3 : n_verts / 3;
    if (n_tris > (1 << 27)) { ctx->err = "mesh too large"; return SHS_ERR_INVALID; }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    // read_v's defaults (rasterizer.hpp:196-202) materialised: normal (0,1,0), uv (0,0)
    std::vector<float> nrm((size_t)n_verts * 3), uv((size_t)n_verts * 2, 0.0f);
    for (int32_t i = 0; i < n_verts; ++i) {
        const bool hn = i < n_normals;
        nrm[3 * (size_t)i] = hn ? normals[3 * (size_t)i] : 0.0f;
        nrm[3 * (size_t)i + 1] = hn ? normals[3 * (size_t)i + 1] : 1.0f;
        nrm[3 * (size_t)i + 2] = hn ? normals[3 * (size_t)i + 2] : 0.0f;
        if (i < n_uvs) { uv[2 * (size_t)i] = uvs[2 * (size_t)i]; uv[2 * (size_t)i + 1] = uvs[2 * (size_t)i + 1]; }
    }
    Mesh m;
    m.lib = true;
    m.n_verts = n_verts;
    m.n_tris = (int32_t)n_tris;
    if (indices && n_indices < 3) m.n_tris = 0;
    // a HIP_TRY that returns early frees what this upload already allocated (the mesh is not registered)
    struct Guard {
        Mesh &m;
        bool keep = false;
        ~Guard() {
            if (keep) return;
            for (void *p : {(void *)m.orig, (void *)m.pos, (void *)m.nrm, (void *)m.uv, (void *)m.idx, (void *)m.cbox})
                if (p) (void)hipFree(p);
        }
    } guard{m};
    // Spatial order (meshes over one 256-triangle chunk): the triangles are stored sorted by the Morton
    // code of their centroid, so a setup block's chunk box is tight and a region-sharded rank skips the
    // blocks that miss its rectangle.  The submission order stays the MeshData order:
    // `orig` gives every stored triangle its MeshData index, the sequence the z ties and the clipped
    // fans are ordered by (rasterizer.hpp:181-442 draws in index order).  A soup's vertices move with
    // their triangle; an indexed mesh keeps its vertices and reorders its index triples.
    const std::vector<uint32_t> order = spatial_order(positions, n_verts, indices, m.n_tris);
    std::vector<float> pos_s, nrm_s, uv_s;
    std::vector<uint32_t> idx_s;
    if (!order.empty()) {
        if (indices) {
            idx_s.resize((size_t)m.n_tris * 3);
            for (size_t p = 0; p < order.size(); ++p)
                for (int k = 0; k < 3; ++k) idx_s[3 * p + k] = indices[3 * (size_t)order[p] + k];
            indices = idx_s.data();
        } else {
            pos_s.assign(positions, positions + (size_t)n_verts * 3);
            nrm_s = nrm;
            uv_s = uv;
            for (size_t p = 0; p < order.size(); ++p)
                for (int k = 0; k < 3; ++k) {
                    const size_t dv = 3 * p + k, sv = 3 * (size_t)order[p] + k;
                    for (int q = 0; q < 3; ++q) { pos_s[3 * dv + q] = positions[3 * sv + q]; nrm_s[3 * dv + q] = nrm[3 * sv + q]; }
                    uv_s[2 * dv] = uv[2 * sv]; uv_s[2 * dv + 1] = uv[2 * sv + 1];
                }
            positions = pos_s.data();
            nrm.swap(nrm_s);
            uv.swap(uv_s);
        }
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m.orig), order.size() * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemcpy(m.orig, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // model-space bounds (PassShadowMap's mesh_bounds_cache, pass_shadow_map.hpp:90-102)
    for (int k = 0; k < 3; ++k) { m.bmin[k] = 3.402823466e38f; m.bmax[k] = -3.402823466e38f; }
    for (int32_t i = 0; i < n_verts; ++i)
        for (int k = 0; k < 3; ++k) {
            const float p = positions[3 * (size_t)i + k];
            m.bmin[k] = (p < m.bmin[k]) ? p : m.bmin[k];   // glm::min(bmin, p)
            m.bmax[k] = (m.bmax[k] < p) ? p : m.bmax[k];   // glm::max(bmax, p)
        }
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m.pos), (size_t)n_verts * 3 * sizeof(float)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m.nrm), (size_t)n_verts * 3 * sizeof(float)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m.uv), (size_t)n_verts * 2 * sizeof(float)));
    HIP_TRY(ctx, hipMemcpy(m.pos, positions, (size_t)n_verts * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(m.nrm, nrm.data(), nrm.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(m.uv, uv.data(), uv.size() * sizeof(float), hipMemcpyHostToDevice));
    if (indices && n_indices >= 3) {
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m.idx), (size_t)n_tris * 3 * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemcpy(m.idx, indices, (size_t)n_tris * 3 * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (m.n_tris > 0) {
        const std::vector<float4> cb = chunk_boxes(positions, n_verts, indices, m.n_tris);
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m.cbox), cb.size() * sizeof(float4)));
        HIP_TRY(ctx, hipMemcpy(m.cbox, cb.data(), cb.size() * sizeof(float4), hipMemcpyHostToDevice));
    }
    m.live = true;
    ctx->meshes.push_back(m);
    guard.keep = true;
    *mesh_id = (int32_t)ctx->meshes.size() - 1;
    return SHS_OK;
}

int shs_texture_upload(shs_ctx *ctx, const uint8_t *rgba, int32_t w, int32_t h, int32_t *tex_id) {
    if (!ctx || !rgba || !tex_id || w <= 0 || h <= 0 || (int64_t)w * h > (1ll << 28)) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    Texture t;
    const size_t bytes = (size_t)w * h * 4;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&t.texels), bytes));
    const hipError_t e = hipMemcpy(t.texels, rgba, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(t.texels);
        ctx->err = hipGetErrorString(e);
        return SHS_ERR_HIP;
    }
    t.w = w;
    t.h = h;
    t.live = true;
    // a released slot is reused (ids stay small); TextureAssetHandle convention: 1-based, 0 = none
    size_t slot = 0;
    while (slot < ctx->textures.size() && ctx->textures[slot].live) ++slot;
    if (slot == ctx->textures.size()) ctx->textures.push_back(t);
    else ctx->textures[slot] = t;
    *tex_id = (int32_t)slot + 1;
    return SHS_OK;
}

int shs_texture_release(shs_ctx *ctx, int32_t tex_id) {
    if (!ctx || tex_id <= 0 || tex_id > (int32_t)ctx->textures.size() || !ctx->textures[(size_t)tex_id - 1].live)
        return SHS_ERR_INVALID;
    if (ctx->sky.model == shs_dev::SKY_CUBEMAP)
        for (int32_t id : ctx->sky_face_tex)
            if (id == tex_id) { ctx->err = "texture is a face of the current sky (shs_lib_set_sky another first)"; return SHS_ERR_INVALID; }
    if (ctx->rt_sky.model == SHS_RT_SKY_CUBEMAP)
        for (int32_t id : ctx->rt_sky.face_tex)
            if (id == tex_id) { ctx->err = "texture is a face of the render-target sky (shs_rt_set_sky another first)"; return SHS_ERR_INVALID; }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    {   // a legacy batch in flight may sample it (SHS_SHADING_TEXTURED): its raster is launched and, should
        // it have overflowed a capacity, re-issued while the texture still exists -- as a mesh's release
        const int rc = shs_legacy_ensure_final(ctx);
        if (rc) return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->setup_stream));
    Texture &t = ctx->textures[(size_t)tex_id - 1];
    HIP_TRY(ctx, hipFree(t.texels));
    t = Texture{};
    return SHS_OK;
}

}  // extern "C"
