// shs_abi_canvas_fx.cpp -- C ABI of the Canvas-API post passes (include/shs_gpu.h; kernels in shs_canvas_fx.hip),
// paths relative to cpp-folders/src/hello-render-target/:
//   shs_canvas_velocity_blur, _fog, _outline, _fxaa          hello_multi_pass.cpp's passes;
//   shs_canvas_spec_bright, _additive, _lens_flare           hello_glowing_star.cpp's;
//   shs_canvas_multi_pass_frame                              hello_multi_pass.cpp:1379-1426 and
//                                                            hello_camera_and_perobject_motion_blur.cpp:1544-1606;
//   shs_canvas_glow_frame                                    hello_glowing_star.cpp:1233-1310;
//   shs_canvas_object_blur                                   hello_per_object_motion_blur.cpp's post_process_motion_blur :461-552;
//   shs_canvas_ping_pong_blur                                hello_ping_pong.cpp:611-618.
// Every entry checks all of its input first, so a rejected call enqueues nothing.  Host buffers are staged through
// the context's device buffers and the call is synchronous; device buffers (SHS_CANVAS_DEVICE) are used in place
// and the call only enqueues.  What does not depend on the pixel is derived here, each a single float operation of
// the reference.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "shs_canvas_fx_internal.hpp"
#include "shs_canvas_post_internal.hpp"
#include "shs_ctx.hpp"

namespace {

using shs_dev::CanvasBrightParams;
using shs_dev::CanvasFlareParams;
using shs_dev::CanvasFogParams;
using shs_dev::CanvasFxaaParams;
using shs_dev::CanvasOutlineParams;
using shs_dev::CanvasVBlurParams;

bool fail(shs_ctx *ctx, const char *msg) {
    ctx->err = msg;
    return false;
}

bool frame_ok(shs_ctx *ctx, int W, int H, uint32_t flags) {
    if (!(W > 0 && H > 0 && W <= 32767 && H <= 32767)) return fail(ctx, "canvas size: 1 .. 32767 per side");
    if (flags & ~SHS_CANVAS_DEVICE) return fail(ctx, "canvas pass flags: SHS_CANVAS_DEVICE only");
    return true;
}

bool all_finite(std::initializer_list<float> v) {
    for (float f : v)
        if (!std::isfinite(f)) return false;
    return true;
}

// the W*H*4 bytes at a and at b share a byte
bool overlap(const void *a, const void *b, size_t npx) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b), n = npx * 4;
    return pa < pb + n && pb < pa + n;
}

bool vblur_ok(shs_ctx *ctx, const shs_canvas_velocity_blur_desc &d) {
    return all_finite({d.strength}) || fail(ctx, "velocity blur: a non-finite strength");
}

bool fog_ok(shs_ctx *ctx, const shs_canvas_fog_desc &d) {
    if (!all_finite({d.fog_start, d.fog_end, d.fog_power})) return fail(ctx, "fog: a non-finite parameter");
    const float den = d.fog_end - d.fog_start;
    return (std::isfinite(den) && den != 0.0f) || fail(ctx, "fog: fog_end - fog_start is zero or not finite");
}

bool outline_ok(shs_ctx *ctx, const shs_canvas_outline_desc &d) {
    if (!all_finite({d.threshold, d.strength})) return fail(ctx, "outline: a non-finite parameter");
    return (d.radius >= 0 && d.radius <= SHS_CANVAS_MAX_OUTLINE_RADIUS) ||
           fail(ctx, "outline: radius 0 .. SHS_CANVAS_MAX_OUTLINE_RADIUS");
}

bool fxaa_ok(shs_ctx *ctx, const shs_canvas_fxaa_desc &d) {
    return all_finite({d.reduce_min, d.reduce_mul, d.span_max}) || fail(ctx, "fxaa: a non-finite parameter");
}

bool bright_ok(shs_ctx *ctx, const shs_canvas_spec_bright_desc &d) {
    return all_finite({d.threshold, d.intensity}) || fail(ctx, "bright pass: a non-finite parameter");
}

bool flare_ok(shs_ctx *ctx, const shs_canvas_lens_flare_desc &d) {
    if (!(d.n_ghosts >= 1 && d.n_ghosts <= SHS_CANVAS_MAX_FLARE_GHOSTS))
        return fail(ctx, "lens flare: n_ghosts 1 .. SHS_CANVAS_MAX_FLARE_GHOSTS");
    bool finite = all_finite({d.intensity, d.halo_intensity, d.chroma_shift_px});
    for (int k = 0; k < d.n_ghosts; ++k) finite = finite && std::isfinite(d.ghost_scales[k]);
    return finite || fail(ctx, "lens flare: a non-finite parameter or ghost scale");
}

bool dof_ok(shs_ctx *ctx, const shs_canvas_dof_desc &d) {   // shs_canvas_dof's own checks
    return (d.blur_iterations >= 0 && d.autofocus_radius >= 0 && d.autofocus_radius <= SHS_CANVAS_MAX_AUTOFOCUS_RADIUS) ||
           fail(ctx, "dof: blur_iterations >= 0, autofocus_radius 0 .. SHS_CANVAS_MAX_AUTOFOCUS_RADIUS");
}

// ---- the passes over device buffers (the descs are checked) -----------------------------------------------------

int run_vblur(shs_ctx *ctx, const shs_canvas_velocity_blur_desc &d, int W, int H, const uint32_t *src, const float *vel,
              uint32_t *dst) {
    CanvasVBlurParams p{};
    p.src = src;
    p.velocity = reinterpret_cast<const float2 *>(vel);
    p.dst = dst;
    p.W = W;
    p.H = H;
    p.samples = d.samples;
    p.strength = d.strength;
    HIP_TRY(ctx, shs_internal::launch_canvas_velocity_blur(p, ctx->stream));
    return SHS_OK;
}

int run_fog(shs_ctx *ctx, const shs_canvas_fog_desc &d, int W, int H, const uint32_t *src, const float *depth, uint32_t *dst,
            float4 *pq) {
    CanvasFogParams p{};
    p.src = src;
    p.depth = depth;
    p.dst = dst;
    p.pq = pq;
    p.W = W;
    p.H = H;
    std::memcpy(&p.fog_rgba, d.fog_color, 4);
    p.start = d.fog_start;
    p.den = d.fog_end - d.fog_start;
    p.power = d.fog_power;
    HIP_TRY(ctx, shs_internal::launch_canvas_fog(p, ctx->stream));
    return SHS_OK;
}

int run_outline(shs_ctx *ctx, const shs_canvas_outline_desc &d, int W, int H, const uint32_t *src, const float *depth,
                uint32_t *dst) {
    CanvasOutlineParams p{};
    p.src = src;
    p.depth = depth;
    p.dst = dst;
    p.W = W;
    p.H = H;
    p.radius = d.radius;
    p.threshold = d.threshold;
    p.strength = d.strength;
    HIP_TRY(ctx, shs_internal::launch_canvas_outline(p, ctx->stream));
    return SHS_OK;
}

int run_fxaa(shs_ctx *ctx, const shs_canvas_fxaa_desc &d, int W, int H, const uint32_t *src, uint32_t *dst) {
    CanvasFxaaParams p{};
    p.src = src;
    p.dst = dst;
    p.W = W;
    p.H = H;
    p.reduce_min = d.reduce_min;
    p.reduce_k = 0.25f * d.reduce_mul;
    p.span_max = d.span_max;
    HIP_TRY(ctx, shs_internal::launch_canvas_fxaa(p, ctx->stream));
    return SHS_OK;
}

int run_bright(shs_ctx *ctx, const shs_canvas_spec_bright_desc &d, int W, int H, const float *spec, uint32_t *dst) {
    CanvasBrightParams p{};
    p.spec = spec;
    p.dst = dst;
    p.W = W;
    p.H = H;
    p.threshold = d.threshold;
    p.den = std::max(1e-6f, 1.0f - d.threshold);
    p.intensity = d.intensity;
    HIP_TRY(ctx, shs_internal::launch_canvas_spec_bright(p, ctx->stream));
    return SHS_OK;
}

int run_flare(shs_ctx *ctx, const shs_canvas_lens_flare_desc &d, int W, int H, const uint32_t *src, uint32_t *dst, float4 *pq) {
    CanvasFlareParams p{};
    p.src = src;
    p.dst = dst;
    p.pq = pq;
    p.W = W;
    p.H = H;
    p.n_ghosts = d.n_ghosts;
    p.cx = 0.5f * float(W);
    p.cy = 0.5f * float(H);
    p.nd_den = std::max(1.0f, std::min(p.cx, p.cy));
    p.intensity = d.intensity;
    p.halo = d.halo_intensity;
    p.chroma = d.chroma_shift_px;
    for (int k = 0; k < d.n_ghosts; ++k) {
        p.scale[k] = d.ghost_scales[k];
        p.weight[k] = 0.45f + 0.55f * (1.0f - float(k) / float(d.n_ghosts));
    }
    HIP_TRY(ctx, shs_internal::launch_canvas_lens_flare(p, ctx->stream));
    return SHS_OK;
}

// ---- host buffers through the context's device buffers; device buffers as they are -------------------------------

template <typename T>
int stage_in(shs_ctx *ctx, bool dev, DevBuf<T> &buf, const void *host, size_t n, const T *&out) {
    if (dev) {
        out = static_cast<const T *>(host);
        return SHS_OK;
    }
    if (ensure(ctx, buf, n)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    out = buf.p;
    return SHS_OK;
}

// where the pass writes: the caller's device buffer, or buf (null target: no such output)
template <typename T>
int stage_out(shs_ctx *ctx, bool dev, DevBuf<T> &buf, void *target, size_t n, T *&out) {
    out = nullptr;
    if (!target) return SHS_OK;
    if (dev) {
        out = static_cast<T *>(target);
        return SHS_OK;
    }
    if (ensure(ctx, buf, n)) return SHS_ERR_HIP;
    out = buf.p;
    return SHS_OK;
}

template <typename T>
int stage_back(shs_ctx *ctx, bool dev, const T *from, void *target, size_t n) {
    if (dev || !target) return SHS_OK;
    HIP_TRY(ctx, hipMemcpyAsync(target, from, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return SHS_OK;
}

int finish(shs_ctx *ctx, bool dev) {
    if (!dev) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SHS_OK;
}

#define TRY(expr)                      \
    do {                               \
        const int rc_ = (expr);        \
        if (rc_ != SHS_OK) return rc_; \
    } while (0)

int fill_black(shs_ctx *ctx, uint32_t *dst, size_t npx) {   // buffer().clear(shs::Color{0, 0, 0, 255})
    HIP_TRY(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dst), (int)0xff000000u, npx, ctx->stream));
    return SHS_OK;
}

}  // namespace

extern "C" {

int shs_canvas_velocity_blur(shs_ctx *ctx, const shs_canvas_velocity_blur_desc *d, const uint8_t *src, const float *velocity,
                             uint8_t *dst, uint32_t flags) {
    if (!ctx || !d || !src || !velocity || !dst) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, d->width, d->height, flags) || !vblur_ok(ctx, *d)) return SHS_ERR_INVALID;
    const size_t npx = (size_t)d->width * d->height;
    if (overlap(src, dst, npx)) return fail(ctx, "velocity blur: dst overlaps src"), SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    const uint32_t *s;
    const float *v;
    uint32_t *o;
    TRY(stage_in(ctx, dev, ctx->cp_a, src, npx, s));
    TRY(stage_in(ctx, dev, ctx->cp_vel, velocity, 2 * npx, v));
    TRY(stage_out(ctx, dev, ctx->cp_b, dst, npx, o));
    TRY(run_vblur(ctx, *d, d->width, d->height, s, v, o));
    TRY(stage_back(ctx, dev, o, dst, npx));
    return finish(ctx, dev);
}

int shs_canvas_fog(shs_ctx *ctx, const shs_canvas_fog_desc *d, const uint8_t *src, const float *depth, uint8_t *dst,
                   float *prequant, uint32_t flags) {
    if (!ctx || !d || !src || !depth || !dst) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, d->width, d->height, flags) || !fog_ok(ctx, *d)) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t npx = (size_t)d->width * d->height;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    const uint32_t *s;
    const float *z;
    uint32_t *o;
    float4 *pq;
    TRY(stage_in(ctx, dev, ctx->cp_a, src, npx, s));
    TRY(stage_in(ctx, dev, ctx->cp_depth, depth, npx, z));
    TRY(stage_out(ctx, dev, ctx->cp_b, dst, npx, o));
    TRY(stage_out(ctx, dev, ctx->cp_pq, prequant, npx, pq));
    TRY(run_fog(ctx, *d, d->width, d->height, s, z, o, pq));
    TRY(stage_back(ctx, dev, o, dst, npx));
    TRY(stage_back(ctx, dev, pq, prequant, npx));
    return finish(ctx, dev);
}

int shs_canvas_outline(shs_ctx *ctx, const shs_canvas_outline_desc *d, const uint8_t *src, const float *depth, uint8_t *dst,
                       uint32_t flags) {
    if (!ctx || !d || !src || !depth || !dst) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, d->width, d->height, flags) || !outline_ok(ctx, *d)) return SHS_ERR_INVALID;
    const size_t npx = (size_t)d->width * d->height;
    if (overlap(src, dst, npx)) return fail(ctx, "outline: dst overlaps src"), SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    const uint32_t *s;
    const float *z;
    uint32_t *o;
    TRY(stage_in(ctx, dev, ctx->cp_a, src, npx, s));
    TRY(stage_in(ctx, dev, ctx->cp_depth, depth, npx, z));
    TRY(stage_out(ctx, dev, ctx->cp_b, dst, npx, o));
    TRY(run_outline(ctx, *d, d->width, d->height, s, z, o));
    TRY(stage_back(ctx, dev, o, dst, npx));
    return finish(ctx, dev);
}

int shs_canvas_fxaa(shs_ctx *ctx, const shs_canvas_fxaa_desc *d, const uint8_t *src, uint8_t *dst, uint32_t flags) {
    if (!ctx || !d || !src || !dst) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, d->width, d->height, flags) || !fxaa_ok(ctx, *d)) return SHS_ERR_INVALID;
    const size_t npx = (size_t)d->width * d->height;
    if (overlap(src, dst, npx)) return fail(ctx, "fxaa: dst overlaps src"), SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    const uint32_t *s;
    uint32_t *o;
    TRY(stage_in(ctx, dev, ctx->cp_a, src, npx, s));
    TRY(stage_out(ctx, dev, ctx->cp_b, dst, npx, o));
    TRY(run_fxaa(ctx, *d, d->width, d->height, s, o));
    TRY(stage_back(ctx, dev, o, dst, npx));
    return finish(ctx, dev);
}

int shs_canvas_spec_bright(shs_ctx *ctx, const shs_canvas_spec_bright_desc *d, const float *spec01, uint8_t *dst,
                           uint32_t flags) {
    if (!ctx || !d || !spec01 || !dst) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, d->width, d->height, flags) || !bright_ok(ctx, *d)) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t npx = (size_t)d->width * d->height;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    const float *s;
    uint32_t *o;
    TRY(stage_in(ctx, dev, ctx->cp_depth, spec01, npx, s));
    TRY(stage_out(ctx, dev, ctx->cp_b, dst, npx, o));
    TRY(run_bright(ctx, *d, d->width, d->height, s, o));
    TRY(stage_back(ctx, dev, o, dst, npx));
    return finish(ctx, dev);
}

int shs_canvas_additive(shs_ctx *ctx, int32_t width, int32_t height, const uint8_t *base, const uint8_t *add, float strength,
                        uint8_t *out, uint32_t flags) {
    if (!ctx || !base || !add || !out) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, width, height, flags)) return SHS_ERR_INVALID;
    if (!std::isfinite(strength)) return fail(ctx, "additive: a non-finite strength"), SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t npx = (size_t)width * height;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    const uint32_t *a, *b;
    uint32_t *o;
    TRY(stage_in(ctx, dev, ctx->cp_a, base, npx, a));
    TRY(stage_in(ctx, dev, ctx->cp_src, add, npx, b));
    TRY(stage_out(ctx, dev, ctx->cp_b, out, npx, o));
    HIP_TRY(ctx, shs_internal::launch_canvas_additive(a, b, o, width, height, strength, ctx->stream));
    TRY(stage_back(ctx, dev, o, out, npx));
    return finish(ctx, dev);
}

int shs_canvas_lens_flare(shs_ctx *ctx, const shs_canvas_lens_flare_desc *d, const uint8_t *src, uint8_t *dst, float *prequant,
                          uint32_t flags) {
    if (!ctx || !d || !src || !dst) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, d->width, d->height, flags) || !flare_ok(ctx, *d)) return SHS_ERR_INVALID;
    const size_t npx = (size_t)d->width * d->height;
    if (overlap(src, dst, npx)) return fail(ctx, "lens flare: dst overlaps src"), SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    const uint32_t *s;
    uint32_t *o;
    float4 *pq;
    TRY(stage_in(ctx, dev, ctx->cp_a, src, npx, s));
    TRY(stage_out(ctx, dev, ctx->cp_b, dst, npx, o));
    TRY(stage_out(ctx, dev, ctx->cp_pq, prequant, npx, pq));
    TRY(run_flare(ctx, *d, d->width, d->height, s, o, pq));
    TRY(stage_back(ctx, dev, o, dst, npx));
    TRY(stage_back(ctx, dev, pq, prequant, npx));
    return finish(ctx, dev);
}

int shs_canvas_object_blur(shs_ctx *ctx, const shs_canvas_object_blur_desc *d, const uint8_t *src, const float *depth,
                           const float *velocity, uint8_t *dst, uint32_t flags) {
    if (!ctx || !d || !src || !depth || !velocity || !dst) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, d->width, d->height, flags)) return SHS_ERR_INVALID;
    if (!all_finite({d->multiplier, d->velocity_scale, d->min_vel2, d->depth_eps}))
        return fail(ctx, "object blur: a non-finite parameter"), SHS_ERR_INVALID;
    if (!(d->max_samples >= 2 && d->max_samples <= SHS_CANVAS_MAX_OBJECT_BLUR_SAMPLES))
        return fail(ctx, "object blur: max_samples 2 .. SHS_CANVAS_MAX_OBJECT_BLUR_SAMPLES"), SHS_ERR_INVALID;
    if (d->depth_rows != 0 && d->depth_rows != 1) return fail(ctx, "object blur: depth_rows is 0 (canvas rows) or 1 (screen rows)"), SHS_ERR_INVALID;
    const size_t npx = (size_t)d->width * d->height;
    if (overlap(src, dst, npx)) return fail(ctx, "object blur: dst overlaps src"), SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    shs_dev::CanvasObjBlurParams p{};
    const float *v;
    TRY(stage_in(ctx, dev, ctx->cp_a, src, npx, p.src));
    TRY(stage_in(ctx, dev, ctx->cp_depth, depth, npx, p.depth));
    TRY(stage_in(ctx, dev, ctx->cp_vel, velocity, 2 * npx, v));
    TRY(stage_out(ctx, dev, ctx->cp_b, dst, npx, p.dst));
    p.velocity = reinterpret_cast<const float2 *>(v);
    p.W = d->width;
    p.H = d->height;
    p.max_samples = d->max_samples;
    p.depth_rows = d->depth_rows;
    p.scale = d->multiplier * d->velocity_scale;   // (BLUR_MULTIPLIER * velocity_scale) :495
    p.min_vel2 = d->min_vel2;
    p.depth_eps = d->depth_eps;
    HIP_TRY(ctx, shs_internal::launch_canvas_object_blur(p, ctx->stream));
    TRY(stage_back(ctx, dev, p.dst, dst, npx));
    return finish(ctx, dev);
}

int shs_canvas_ping_pong_blur(shs_ctx *ctx, int32_t width, int32_t height, int32_t iterations, uint8_t *color, uint32_t flags) {
    if (!ctx || !color) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, width, height, flags)) return SHS_ERR_INVALID;
    if (iterations < 0) return fail(ctx, "ping-pong blur: iterations >= 0"), SHS_ERR_INVALID;
    if (iterations == 0) return SHS_OK;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t npx = (size_t)width * height;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    if (ensure(ctx, ctx->fx_pong, npx)) return SHS_ERR_HIP;
    uint32_t *ping = reinterpret_cast<uint32_t *>(color), *pong = ctx->fx_pong.p;
    if (!dev) {
        if (ensure(ctx, ctx->cp_a, npx)) return SHS_ERR_HIP;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->cp_a.p, color, npx * 4, hipMemcpyHostToDevice, ctx->stream));
        ping = ctx->cp_a.p;
    }
    for (int it = 0; it < iterations; ++it) {   // ping -> pong horizontal, pong -> ping vertical (:615-616)
        HIP_TRY(ctx, shs_internal::launch_canvas_gaussian(ping, pong, width, height, true, ctx->stream));
        HIP_TRY(ctx, shs_internal::launch_canvas_gaussian(pong, ping, width, height, false, ctx->stream));
    }
    TRY(stage_back(ctx, dev, ping, color, npx));
    return finish(ctx, dev);
}

// The chains run on device buffers: host inputs are staged into fx_in / fx_depth / fx_vel / fx_spec, the frame is
// written to fx_out and copied back.  fx_a, fx_b, fx_c are the demos' intermediate canvases; the DoF step and the
// combined motion blur are the existing entries over device buffers (cp_a, cp_b and cp_focus are the DoF's own).
int shs_canvas_multi_pass_frame(shs_ctx *ctx, const shs_canvas_multi_pass_frame_desc *d, const uint8_t *color, const float *depth,
                                const float *velocity, uint8_t *dst, uint32_t flags) {
    if (!ctx || !d || !color || !depth || !velocity || !dst) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, d->width, d->height, flags)) return SHS_ERR_INVALID;
    if (d->blur_mode < SHS_CANVAS_BLUR_VELOCITY_FIRST || d->blur_mode > SHS_CANVAS_BLUR_COMBINED_LATE)
        return fail(ctx, "multi-pass frame: blur_mode is one of SHS_CANVAS_BLUR_*"), SHS_ERR_INVALID;
    if (d->blur_mode == SHS_CANVAS_BLUR_VELOCITY_FIRST && !vblur_ok(ctx, d->velocity_blur)) return SHS_ERR_INVALID;
    if ((d->enable_dof && !dof_ok(ctx, d->dof)) || !fog_ok(ctx, d->fog) || !outline_ok(ctx, d->outline) ||
        (d->enable_fxaa && !fxaa_ok(ctx, d->fxaa)))
        return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const int W = d->width, H = d->height;
    const size_t npx = (size_t)W * H;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    const uint32_t *in;
    const float *z, *vel;
    uint32_t *out;
    TRY(stage_in(ctx, dev, ctx->fx_in, color, npx, in));
    TRY(stage_in(ctx, dev, ctx->fx_depth, depth, npx, z));
    TRY(stage_in(ctx, dev, ctx->fx_vel, velocity, 2 * npx, vel));
    TRY(stage_out(ctx, dev, ctx->fx_out, dst, npx, out));
    if (ensure(ctx, ctx->fx_a, npx) || ensure(ctx, ctx->fx_b, npx)) return SHS_ERR_HIP;
    uint32_t *A = ctx->fx_a.p, *B = ctx->fx_b.p;
    shs_canvas_motion_blur_desc mb = d->motion_blur;
    mb.width = W;
    mb.height = H;
    shs_canvas_dof_desc dof = d->dof;
    dof.width = W;
    dof.height = H;
    auto combined_blur = [&](const uint32_t *s, uint32_t *o) {
        return shs_canvas_motion_blur(ctx, &mb, reinterpret_cast<const uint8_t *>(s), z, vel, reinterpret_cast<uint8_t *>(o),
                                      SHS_CANVAS_DEVICE);
    };
    auto dof_step = [&](uint32_t *c) {
        return shs_canvas_dof(ctx, &dof, reinterpret_cast<uint8_t *>(c), z, nullptr, nullptr, SHS_CANVAS_DEVICE);
    };
    if (d->blur_mode == SHS_CANVAS_BLUR_COMBINED_LATE) {
        const uint32_t *cur = in;
        if (d->enable_dof) {   // sharp_copy = rt_scene.color
            HIP_TRY(ctx, hipMemcpyAsync(A, in, npx * 4, hipMemcpyDeviceToDevice, ctx->stream));
            TRY(dof_step(A));
            cur = A;
        }
        TRY(run_fog(ctx, d->fog, W, H, cur, z, B, nullptr));
        TRY(run_outline(ctx, d->outline, W, H, B, z, A));
        TRY(combined_blur(A, d->enable_fxaa ? B : out));
        if (d->enable_fxaa) TRY(run_fxaa(ctx, d->fxaa, W, H, B, out));
    } else {
        if (d->blur_mode == SHS_CANVAS_BLUR_VELOCITY_FIRST) TRY(run_vblur(ctx, d->velocity_blur, W, H, in, vel, A));
        else TRY(combined_blur(in, A));
        if (d->enable_dof) TRY(dof_step(A));
        TRY(run_fog(ctx, d->fog, W, H, A, z, B, nullptr));
        TRY(run_outline(ctx, d->outline, W, H, B, z, d->enable_fxaa ? A : out));
        if (d->enable_fxaa) TRY(run_fxaa(ctx, d->fxaa, W, H, A, out));
    }
    TRY(stage_back(ctx, dev, out, dst, npx));
    return finish(ctx, dev);
}

int shs_canvas_glow_frame(shs_ctx *ctx, const shs_canvas_glow_frame_desc *d, const uint8_t *color, const float *depth,
                          const float *velocity, const float *spec01, uint8_t *dst, uint32_t flags) {
    if (!ctx || !d || !color || !depth || !velocity || !spec01 || !dst) return SHS_ERR_INVALID;
    if (!frame_ok(ctx, d->width, d->height, flags) || !vblur_ok(ctx, d->velocity_blur)) return SHS_ERR_INVALID;
    if (d->bloom_iterations < 0) return fail(ctx, "glow frame: bloom_iterations >= 0"), SHS_ERR_INVALID;
    if ((d->enable_dof && !dof_ok(ctx, d->dof)) || (d->enable_bloom && !bright_ok(ctx, d->spec_bright)) ||
        (d->enable_flare && !flare_ok(ctx, d->lens_flare)))
        return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const int W = d->width, H = d->height;
    const size_t npx = (size_t)W * H;
    const bool dev = (flags & SHS_CANVAS_DEVICE) != 0;
    const uint32_t *in;
    const float *z, *vel, *spec;
    uint32_t *out;
    TRY(stage_in(ctx, dev, ctx->fx_in, color, npx, in));
    TRY(stage_in(ctx, dev, ctx->fx_depth, depth, npx, z));
    TRY(stage_in(ctx, dev, ctx->fx_vel, velocity, 2 * npx, vel));
    TRY(stage_in(ctx, dev, ctx->fx_spec, spec01, npx, spec));
    TRY(stage_out(ctx, dev, ctx->fx_out, dst, npx, out));
    if (ensure(ctx, ctx->fx_a, npx) || ensure(ctx, ctx->fx_b, npx) || ensure(ctx, ctx->fx_c, npx)) return SHS_ERR_HIP;
    uint32_t *dof_out = ctx->fx_a.p, *bloom = ctx->fx_b.p, *flare = ctx->fx_c.p;
    TRY(run_vblur(ctx, d->velocity_blur, W, H, in, vel, dof_out));
    if (d->enable_dof) {
        shs_canvas_dof_desc dof = d->dof;
        dof.width = W;
        dof.height = H;
        TRY(shs_canvas_dof(ctx, &dof, reinterpret_cast<uint8_t *>(dof_out), z, nullptr, nullptr, SHS_CANVAS_DEVICE));
    }
    if (d->enable_bloom) {   // bloom_pong = bright_spec; per iteration horizontal pong -> ping, vertical ping -> pong
        TRY(run_bright(ctx, d->spec_bright, W, H, spec, bloom));
        for (int it = 0; it < d->bloom_iterations; ++it) {
            HIP_TRY(ctx, shs_internal::launch_canvas_gaussian(bloom, flare, W, H, true, ctx->stream));
            HIP_TRY(ctx, shs_internal::launch_canvas_gaussian(flare, bloom, W, H, false, ctx->stream));
        }
    } else {
        TRY(fill_black(ctx, bloom, npx));
    }
    if (d->enable_flare) TRY(run_flare(ctx, d->lens_flare, W, H, bloom, flare, nullptr));
    else TRY(fill_black(ctx, flare, npx));
    HIP_TRY(ctx, shs_internal::launch_canvas_additive(dof_out, bloom, out, W, H, 1.0f, ctx->stream));
    HIP_TRY(ctx, shs_internal::launch_canvas_additive(out, flare, out, W, H, 1.0f, ctx->stream));
    TRY(stage_back(ctx, dev, out, dst, npx));
    return finish(ctx, dev);
}

}  // extern "C"
