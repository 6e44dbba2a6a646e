// shs_abi_sky.cpp -- the sky models of the library path (include/shs_gpu.h): the scene's sky description
// (shs_lib_set_sky) and shs_sky_sample.  Reference paths are relative to shs-renderer-lib/include/shs/.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/shs_gpu.h"
#include "shs_ctx.hpp"
#include "shs_glm.hpp"
#include "shs_lib_host.hpp"
#include "shs_lib_internal.hpp"

using shs_lib_host::ensure_srgb_lut;

// shs_sky_desc -> the kernels' SkyParams.  camera: with the unprojection's fields (shs_lib_set_sky), which
// shs_sky_sample does not read.
static int build_sky(shs_ctx *ctx, const shs_sky_desc &d, bool camera, shs_dev::SkyParams &o) {
    std::memset(&o, 0, sizeof o);
    if (d.model != SHS_SKY_PROCEDURAL && d.model != SHS_SKY_CUBEMAP) { ctx->err = "sky model: SHS_SKY_PROCEDURAL or SHS_SKY_CUBEMAP"; return SHS_ERR_INVALID; }
    o.model = d.model == SHS_SKY_PROCEDURAL ? shs_dev::SKY_PROCEDURAL : shs_dev::SKY_CUBEMAP;
    if (camera) {
        bool finite = true;
        for (float v : d.cam_viewproj) finite = finite && std::isfinite(v);
        for (float v : d.cam_pos) finite = finite && std::isfinite(v);
        if (!finite) { ctx->err = "sky cam_viewproj / cam_pos must be finite"; return SHS_ERR_INVALID; }
        shs_host::inverse(d.cam_viewproj, o.inv_vp);   // skybox_renderer.hpp:29
        for (float v : o.inv_vp) finite = finite && std::isfinite(v);
        if (!finite) { ctx->err = "sky cam_viewproj has no finite inverse"; return SHS_ERR_INVALID; }
        for (int i = 0; i < 3; ++i) o.cam[i] = d.cam_pos[i];
    }
    if (d.model == SHS_SKY_PROCEDURAL) {
        if (!(std::isfinite(d.sun_dir_ws[0]) && std::isfinite(d.sun_dir_ws[1]) && std::isfinite(d.sun_dir_ws[2]))) {
            ctx->err = "sky sun_dir_ws must be finite";
            return SHS_ERR_INVALID;
        }
        // procedural_sky.hpp:23
        const shs_host::vec3 s = shs_host::gnormalize(shs_host::vec3{d.sun_dir_ws[0], d.sun_dir_ws[1], d.sun_dir_ws[2]});
        if (!(std::isfinite(s.x) && std::isfinite(s.y) && std::isfinite(s.z))) { ctx->err = "sky sun_dir_ws cannot be normalised"; return SHS_ERR_INVALID; }
        o.sun[0] = s.x; o.sun[1] = s.y; o.sun[2] = s.z;
    } else {
        if (!std::isfinite(d.intensity)) { ctx->err = "sky intensity must be finite"; return SHS_ERR_INVALID; }
        o.intensity = d.intensity;
        for (int k = 0; k < 6; ++k) {
            const int32_t id = d.face_tex[k];
            if (id <= 0 || id > (int32_t)ctx->textures.size() || !ctx->textures[(size_t)id - 1].live) {
                ctx->err = "sky face_tex (not a live texture id)";
                return SHS_ERR_INVALID;
            }
            const Texture &t = ctx->textures[(size_t)id - 1];
            o.face[k] = t.texels;
            o.fw[k] = t.w;
            o.fh[k] = t.h;
        }
    }
    return SHS_OK;
}

extern "C" {

int shs_lib_set_sky(shs_ctx *ctx, const shs_sky_desc *desc) {
    if (!ctx) return SHS_ERR_INVALID;
    if (!desc || desc->model == SHS_SKY_NONE) {
        ctx->sky = shs_dev::SkyParams{};
        return SHS_OK;
    }
    shs_dev::SkyParams sk;
    const int rc = build_sky(ctx, *desc, true, sk);
    if (rc) return rc;
    if (sk.model == shs_dev::SKY_CUBEMAP) {
        if (set_dev(ctx)) return SHS_ERR_HIP;
        if (ensure_srgb_lut(ctx)) return SHS_ERR_HIP;
    }
    ctx->sky = sk;
    for (int k = 0; k < 6; ++k) ctx->sky_face_tex[k] = desc->face_tex[k];
    return SHS_OK;
}

int shs_sky_sample(shs_ctx *ctx, const shs_sky_desc *desc, const float *dirs3, int32_t n, float *rgb3) {
    if (!ctx || !desc || n < 0 || (n > 0 && (!dirs3 || !rgb3))) return SHS_ERR_INVALID;
    shs_dev::SkyParams sk;
    const int rc = build_sky(ctx, *desc, false, sk);
    if (rc) return rc;
    if (n == 0) return SHS_OK;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    if (ensure_srgb_lut(ctx)) return SHS_ERR_HIP;
    float *buf = nullptr;   // n directions, then n colours
    const size_t bytes = (size_t)n * 3 * sizeof(float);
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&buf), 2 * bytes));
    hipError_t e = hipMemcpy(buf, dirs3, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = shs_internal::launch_sky_sample(sk, ctx->srgb_lut.p, buf, n, buf + (size_t)n * 3, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(rgb3, buf + (size_t)n * 3, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) {
        ctx->err = hipGetErrorString(e);
        return SHS_ERR_HIP;
    }
    return SHS_OK;
}

}  // extern "C"
