// shs_canvas_fx_internal.hpp -- launch interface of shs_canvas_fx.hip: the Canvas-API post passes of
// hello_multi_pass.cpp, hello_glowing_star.cpp and hello_per_object_motion_blur.cpp (paths relative to hello-render-target/).  Buffers indexed
// y * W + x, as the passes index their canvases.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace shs_dev {

constexpr int FX_MAX_GHOSTS = 8;

// motion_blur_pass (hello_multi_pass.cpp:605-683)
struct CanvasVBlurParams {
    const uint32_t *src;
    const float2 *velocity;   // Buffer<glm::vec2> (canvas px)
    uint32_t *dst;
    int32_t W, H, samples;
    float strength;
};

// fog_pass (:764-819), outline_pass (:689-758): colour and the ZBuffer (view z; FLT_MAX = empty)
struct CanvasFogParams {
    const uint32_t *src;
    const float *depth;
    uint32_t *dst;
    float4 *pq;               // may be null
    int32_t W, H;
    uint32_t fog_rgba;
    float start, den;         // den: fog_end - fog_start
    float power;
};

struct CanvasOutlineParams {
    const uint32_t *src;
    const float *depth;
    uint32_t *dst;
    int32_t W, H, radius;
    float threshold, strength;
};

// fxaa_pass (:1000-1114)
struct CanvasFxaaParams {
    const uint32_t *src;
    uint32_t *dst;
    int32_t W, H;
    float reduce_min;
    float reduce_k;           // 0.25f * FXAA_REDUCE_MUL
    float span_max;
};

// build_spec_bright_pass (hello_glowing_star.cpp:700-752)
struct CanvasBrightParams {
    const float *spec;
    uint32_t *dst;
    int32_t W, H;
    float threshold;
    float den;                // std::max(1e-6f, 1.0f - threshold)
    float intensity;
};

// pseudo_lens_flare_pass (hello_glowing_star.cpp:802-906)
struct CanvasFlareParams {
    const uint32_t *src;
    uint32_t *dst;
    float4 *pq;               // may be null
    int32_t W, H, n_ghosts;
    float cx, cy;             // 0.5f * float(W), 0.5f * float(H)
    float nd_den;             // std::max(1.0f, std::min(cx, cy))
    float intensity, halo, chroma;
    float scale[FX_MAX_GHOSTS];
    float weight[FX_MAX_GHOSTS];   // 0.45f + 0.55f * (1.0f - float(i) / float(n_ghosts))
};

// post_process_motion_blur (hello_per_object_motion_blur.cpp:461-552)
struct CanvasObjBlurParams {
    const uint32_t *src;
    const float *depth;       // the ZBuffer's raw plane (FLT_MAX = empty)
    const float2 *velocity;   // Buffer<glm::vec2> (canvas px, +Y up)
    uint32_t *dst;
    int32_t W, H, max_samples;
    int32_t depth_rows;       // 0: depth in canvas rows, read at y; 1: in screen rows, read at H - 1 - y (:508, :524)
    float scale;              // BLUR_MULTIPLIER * velocity_scale
    float min_vel2, depth_eps;
};

}  // namespace shs_dev

namespace shs_internal {
hipError_t launch_canvas_object_blur(const shs_dev::CanvasObjBlurParams &p, hipStream_t s);
hipError_t launch_canvas_velocity_blur(const shs_dev::CanvasVBlurParams &p, hipStream_t s);
hipError_t launch_canvas_fog(const shs_dev::CanvasFogParams &p, hipStream_t s);
hipError_t launch_canvas_outline(const shs_dev::CanvasOutlineParams &p, hipStream_t s);
hipError_t launch_canvas_fxaa(const shs_dev::CanvasFxaaParams &p, hipStream_t s);
hipError_t launch_canvas_spec_bright(const shs_dev::CanvasBrightParams &p, hipStream_t s);
hipError_t launch_canvas_additive(const uint32_t *base, const uint32_t *add, uint32_t *out, int W, int H, float strength,
                                  hipStream_t s);
hipError_t launch_canvas_lens_flare(const shs_dev::CanvasFlareParams &p, hipStream_t s);
}  // namespace shs_internal
