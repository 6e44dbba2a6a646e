// shs_canvas_fx.hip -- the Canvas-API post passes of three render-target demos on gfx950 (paths relative to
// cpp-folders/src/hello-render-target/):
//   k_canvas_velocity_blur  motion_blur_pass (hello_multi_pass.cpp:605-683 = hello_glowing_star.cpp:441-523);
//   k_canvas_fog            fog_pass (hello_multi_pass.cpp:764-819) over smoothstep01 / lerp_color (:120-137);
//   k_canvas_outline        outline_pass (:689-758);
//   k_canvas_fxaa           fxaa_pass (:1000-1114) over luma_from_color (:159-165) and color_from_rgbaf (:139-146);
//   k_canvas_spec_bright    build_spec_bright_pass (hello_glowing_star.cpp:700-752);
//   k_canvas_additive       additive_composite_pass (:754-795) over mul_color / add_color_clamped (:146-164);
//   k_canvas_lens_flare     pseudo_lens_flare_pass (:802-906);
//   k_canvas_object_blur    post_process_motion_blur (hello_per_object_motion_blur.cpp:461-552).
// One thread per pixel over 64 x 4 pixel blocks; every float expression keeps the reference's operands and order
// (-ffp-contract=off, correctly rounded '/' and sqrt), so the output bytes are the reference's.  The two
// transcendentals -- the fog's std::pow and the flare's std::exp -- are the function in double rounded once to
// float (as k_canvas_light_shafts'), where the reference has the host's float libm.
#include <float.h>
#include <limits.h>

#include "shs_canvas_fx_internal.hpp"

namespace shs_dev {

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return (v < lo) ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return (v < lo) ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float s_min(float a, float b) { return (b < a) ? b : a; }   // std::min
__device__ __forceinline__ float s_max(float a, float b) { return (a < b) ? b : a; }   // std::max
// (int)f as the reference's x86-64 build converts it (cvttss2si: NaN and out-of-range give INT_MIN, which every
// caller's clamp brings to its lower bound)
__device__ __forceinline__ int int_x86(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN; }
__device__ __forceinline__ int round_i(float v) { return int_x86(roundf(v)); }   // (int)std::round(v)
__device__ __forceinline__ float smoothstep01(float t) {
    t = clampf(t, 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}
__device__ __forceinline__ uint32_t pack(int r, int g, int b, int a) {
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | ((uint32_t)a << 24);
}
__device__ __forceinline__ float chan(uint32_t c, int ch) { return (float)((c >> (8 * ch)) & 0xffu); }
// one channel of color_from_rgbaf: the clamp, then x86's float -> uint8_t
__device__ __forceinline__ uint32_t byte_f(float v) { return (uint32_t)(uint8_t)(int)s_min(255.0f, s_max(0.0f, v)); }
__device__ __forceinline__ uint32_t rgbaf(float r, float g, float b) {
    return byte_f(r) | (byte_f(g) << 8) | (byte_f(b) << 16) | (255u << 24);
}
// luma_from_color
__device__ __forceinline__ float luma(uint32_t c) {
    const float r = chan(c, 0) / 255.0f, g = chan(c, 1) / 255.0f, b = chan(c, 2) / 255.0f;
    return 0.299f * r + 0.587f * g + 0.114f * b;
}
// the passes' sample lambdas: clamped texel, and the texel nearest a float position
__device__ __forceinline__ uint32_t tap(const uint32_t *src, int W, int H, int sx, int sy) {
    return src[(size_t)clampi(sy, 0, H - 1) * W + clampi(sx, 0, W - 1)];
}
__device__ __forceinline__ uint32_t tap_f(const uint32_t *src, int W, int H, float fx, float fy) {
    return tap(src, W, H, round_i(fx), round_i(fy));
}

}  // namespace

#define FX_PIXEL(W, H)                                                \
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));      \
    const int y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));        \
    if (x >= (W) || y >= (H)) return;                                 \
    const size_t i = (size_t)y * (W) + x

__global__ __launch_bounds__(256) void k_canvas_velocity_blur(CanvasVBlurParams p) {
    FX_PIXEL(p.W, p.H);
    const float2 vf = p.velocity[i];
    const float vx = vf.x * p.strength, vy = vf.y * p.strength;
    const float vlen = sqrtf(vx * vx + vy * vy);
    if (vlen < 0.001f || p.samples <= 1) {
        p.dst[i] = p.src[i];
        return;
    }
    const float dx = vx / vlen, dy = vy / vlen;
    float r = 0.0f, g = 0.0f, b = 0.0f, wsum = 0.0f;
    for (int k = 0; k < p.samples; ++k) {
        const float t = (float)k / (float)(p.samples - 1);
        const float a = (t - 0.5f) * 2.0f;
        const float al = a * vlen;
        const uint32_t c = tap_f(p.src, p.W, p.H, (float)x + dx * al, (float)y + dy * al);
        const float wgt = 1.0f - fabsf(a);
        r += wgt * chan(c, 0);
        g += wgt * chan(c, 1);
        b += wgt * chan(c, 2);
        wsum += wgt;
    }
    if (wsum < 0.0001f) wsum = 1.0f;
    p.dst[i] = pack(clampi(int_x86(r / wsum), 0, 255), clampi(int_x86(g / wsum), 0, 255), clampi(int_x86(b / wsum), 0, 255), 255);
}

__global__ __launch_bounds__(256) void k_canvas_fog(CanvasFogParams p) {
    FX_PIXEL(p.W, p.H);
    const uint32_t c = p.src[i];
    const float d = p.depth[i];
    if (d == FLT_MAX) {
        p.dst[i] = c;
        if (p.pq) p.pq[i] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        return;
    }
    float t = (d - p.start) / p.den;
    t = smoothstep01(t);
    t = (float)pow((double)t, (double)p.power);
    t = clampf(t, 0.0f, 1.0f);   // lerp_color
    const float ia = 1.0f - t;
    float v[3];
    uint32_t out = 255u << 24;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        v[ch] = ia * chan(c, ch) + t * chan(p.fog_rgba, ch);
        out |= (uint32_t)(uint8_t)(int)v[ch] << (8 * ch);
    }
    p.dst[i] = out;
    if (p.pq) p.pq[i] = make_float4(v[0], v[1], v[2], 1.0f);
}

__global__ __launch_bounds__(256) void k_canvas_outline(CanvasOutlineParams p) {
    FX_PIXEL(p.W, p.H);
    const uint32_t c = p.src[i];
    const float d0 = p.depth[i];
    if (d0 == FLT_MAX) {
        p.dst[i] = c;
        return;
    }
    float max_delta = 0.0f;
    for (int oy = -p.radius; oy <= p.radius; ++oy) {
        const size_t row = (size_t)clampi(y + oy, 0, p.H - 1) * p.W;
        for (int ox = -p.radius; ox <= p.radius; ++ox) {
            if (ox == 0 && oy == 0) continue;
            const float d1 = p.depth[row + clampi(x + ox, 0, p.W - 1)];
            if (d1 == FLT_MAX) continue;
            max_delta = s_max(max_delta, fabsf(d1 - d0));
        }
    }
    const float edge = (max_delta > p.threshold) ? 1.0f : 0.0f;
    const float k = 1.0f - edge * p.strength;
    p.dst[i] = pack(clampi(int_x86(chan(c, 0) * k), 0, 255), clampi(int_x86(chan(c, 1) * k), 0, 255),
                    clampi(int_x86(chan(c, 2) * k), 0, 255), 255);
}

__global__ __launch_bounds__(256) void k_canvas_fxaa(CanvasFxaaParams p) {
    FX_PIXEL(p.W, p.H);
    const uint32_t rgbM = p.src[i];
    const float lumaM = luma(rgbM);
    const float lumaNW = luma(tap(p.src, p.W, p.H, x - 1, y + 1));
    const float lumaNE = luma(tap(p.src, p.W, p.H, x + 1, y + 1));
    const float lumaSW = luma(tap(p.src, p.W, p.H, x - 1, y - 1));
    const float lumaSE = luma(tap(p.src, p.W, p.H, x + 1, y - 1));
    const float lumaMin = s_min(lumaM, s_min(s_min(lumaNW, lumaNE), s_min(lumaSW, lumaSE)));
    const float lumaMax = s_max(lumaM, s_max(s_max(lumaNW, lumaNE), s_max(lumaSW, lumaSE)));
    const float contrast = lumaMax - lumaMin;
    if (contrast < 0.02f) {
        p.dst[i] = rgbM;
        return;
    }
    float dirx = -((lumaNW + lumaNE) - (lumaSW + lumaSE));
    float diry = ((lumaNW + lumaSW) - (lumaNE + lumaSE));
    const float dirReduce = s_max((lumaNW + lumaNE + lumaSW + lumaSE) * p.reduce_k, p.reduce_min);
    const float rcpDirMin = 1.0f / (s_min(fabsf(dirx), fabsf(diry)) + dirReduce);
    dirx = clampf(dirx * rcpDirMin, -p.span_max, p.span_max);
    diry = clampf(diry * rcpDirMin, -p.span_max, p.span_max);
    const float fx = (float)x, fy = (float)y;
    const uint32_t a1 = tap_f(p.src, p.W, p.H, fx + dirx * (1.0f / 3.0f - 0.5f), fy + diry * (1.0f / 3.0f - 0.5f));
    const uint32_t a2 = tap_f(p.src, p.W, p.H, fx + dirx * (2.0f / 3.0f - 0.5f), fy + diry * (2.0f / 3.0f - 0.5f));
    const uint32_t b1 = tap_f(p.src, p.W, p.H, fx + dirx * (0.0f / 3.0f - 0.5f), fy + diry * (0.0f / 3.0f - 0.5f));
    const uint32_t b2 = tap_f(p.src, p.W, p.H, fx + dirx * (3.0f / 3.0f - 0.5f), fy + diry * (3.0f / 3.0f - 0.5f));
    const uint32_t rgbA = rgbaf(0.5f * (chan(a1, 0) + chan(a2, 0)), 0.5f * (chan(a1, 1) + chan(a2, 1)),
                                0.5f * (chan(a1, 2) + chan(a2, 2)));
    const uint32_t rgbB = rgbaf(0.5f * chan(rgbA, 0) + 0.25f * (chan(b1, 0) + chan(b2, 0)),
                                0.5f * chan(rgbA, 1) + 0.25f * (chan(b1, 1) + chan(b2, 1)),
                                0.5f * chan(rgbA, 2) + 0.25f * (chan(b1, 2) + chan(b2, 2)));
    const float lumaB = luma(rgbB);
    p.dst[i] = (lumaB < lumaMin || lumaB > lumaMax) ? rgbA : rgbB;
}

__global__ __launch_bounds__(256) void k_canvas_spec_bright(CanvasBrightParams p) {
    FX_PIXEL(p.W, p.H);
    float v = (p.spec[i] - p.threshold) / p.den;
    v = smoothstep01(v);
    v *= p.intensity;
    // 255.0f * gold.r * v with gold = (1.0f, 0.88f, 0.45f); a NaN v ends at std::max(0.0f, NaN) = 0
    p.dst[i] = rgbaf(255.0f * 1.0f * v, 255.0f * 0.88f * v, 255.0f * 0.45f * v);
}

__global__ __launch_bounds__(256) void k_canvas_additive(const uint32_t *base, const uint32_t *add, uint32_t *out, int W, int H,
                                                         float strength) {
    FX_PIXEL(W, H);
    const uint32_t a = base[i], c = add[i];
    int o[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int b = clampi(int_x86(chan(c, ch) * strength), 0, 255);   // mul_color
        o[ch] = clampi((int)((a >> (8 * ch)) & 0xffu) + b, 0, 255);       // add_color_clamped
    }
    out[i] = pack(o[0], o[1], o[2], 255);
}

__global__ __launch_bounds__(256) void k_canvas_lens_flare(CanvasFlareParams p) {
    FX_PIXEL(p.W, p.H);
    const float dx = (float)x - p.cx, dy = (float)y - p.cy;
    const float dist = sqrtf(dx * dx + dy * dy);
    const float nd = dist / p.nd_den;
    const float vign = 1.0f - smoothstep01(nd);
    float dirx = 0.0f, diry = 0.0f;
    if (dist > 1e-4f) {
        dirx = dx / dist;
        diry = dy / dist;
    }
    const float ox = dirx * p.chroma, oy = diry * p.chroma;
    float rr = 0.0f, gg = 0.0f, bb = 0.0f;
    for (int k = 0; k < p.n_ghosts; ++k) {
        const float s = p.scale[k];
        const float sx = p.cx - dx * s, sy = p.cy - dy * s;
        const uint32_t cR = tap_f(p.src, p.W, p.H, sx + ox, sy + oy);
        const uint32_t cG = tap_f(p.src, p.W, p.H, sx, sy);
        const uint32_t cB = tap_f(p.src, p.W, p.H, sx - ox, sy - oy);
        const float w = p.weight[k];
        rr += w * chan(cR, 0);
        gg += w * chan(cG, 1);
        bb += w * chan(cB, 2);
    }
    {
        const uint32_t hC = tap_f(p.src, p.W, p.H, p.cx - dx * 0.35f, p.cy - dy * 0.35f);
        const float ring = (float)exp((double)(-8.0f * (nd - 0.35f) * (nd - 0.35f)));
        rr += p.halo * ring * chan(hC, 0);
        gg += p.halo * ring * chan(hC, 1);
        bb += p.halo * ring * chan(hC, 2);
    }
    rr *= p.intensity * vign;
    gg *= p.intensity * vign;
    bb *= p.intensity * vign;
    p.dst[i] = rgbaf(rr, gg, bb);
    if (p.pq) p.pq[i] = make_float4(rr, gg, bb, 1.0f);
}

// post_process_motion_blur (hello_per_object_motion_blur.cpp:461-552): a kernel centred on the pixel, as many samples as
// the scaled speed in pixels, each kept where its depth lies within eps of the pixel's; the source pixel where the motion
// is small or nothing survives.  Every index is checked before it is used: a sample outside the canvas is skipped, a
// depth outside it is FLT_MAX.
__global__ __launch_bounds__(256) void k_canvas_object_blur(CanvasObjBlurParams p) {
    FX_PIXEL(p.W, p.H);
    const float2 vf = p.velocity[i];
    const float vx = vf.x * p.scale, vy = vf.y * p.scale;
    const float vv = vx * vx + vy * vy;
    if (vv < p.min_vel2) {
        p.dst[i] = p.src[i];
        return;
    }
    int samples = int_x86(sqrtf(vv));
    if (samples < 2) samples = 2;
    if (samples > p.max_samples) samples = p.max_samples;
    // ZBuffer::get_depth_at at canvas (x, row): the plane's own row is the screen row when depth_rows is set
    const float z0 = p.depth[(size_t)(p.depth_rows ? p.H - 1 - y : y) * p.W + x];
    float r = 0.0f, g = 0.0f, b = 0.0f, wsum = 0.0f;
    for (int k = 0; k < samples; ++k) {
        const float t = (float)k / (float)(samples - 1);
        const float o = t - 0.5f;
        const int sx = int_x86((float)x - vx * o);
        const int sy = int_x86((float)y - vy * o);
        if (sx < 0 || sx >= p.W || sy < 0 || sy >= p.H) continue;
        const float zs = p.depth[(size_t)(p.depth_rows ? p.H - 1 - sy : sy) * p.W + sx];
        if (fabsf(zs - z0) > p.depth_eps) continue;
        const uint32_t c = p.src[(size_t)sy * p.W + sx];
        r += chan(c, 0);
        g += chan(c, 1);
        b += chan(c, 2);
        wsum += 1.0f;
    }
    if (wsum <= 0.0f) {
        p.dst[i] = p.src[i];
        return;
    }
    p.dst[i] = rgbaf(r / wsum, g / wsum, b / wsum);
}

#undef FX_PIXEL

}  // namespace shs_dev

namespace shs_internal {
using namespace shs_dev;

static dim3 px_grid(int W, int H) { return dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)); }

hipError_t launch_canvas_velocity_blur(const CanvasVBlurParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_velocity_blur, px_grid(p.W, p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_canvas_fog(const CanvasFogParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_fog, px_grid(p.W, p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_canvas_outline(const CanvasOutlineParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_outline, px_grid(p.W, p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_canvas_fxaa(const CanvasFxaaParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_fxaa, px_grid(p.W, p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_canvas_spec_bright(const CanvasBrightParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_spec_bright, px_grid(p.W, p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_canvas_additive(const uint32_t *base, const uint32_t *add, uint32_t *out, int W, int H, float strength,
                                  hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_additive, px_grid(W, H), dim3(256), 0, s, base, add, out, W, H, strength);
    return hipGetLastError();
}

hipError_t launch_canvas_lens_flare(const CanvasFlareParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_lens_flare, px_grid(p.W, p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_canvas_object_blur(const CanvasObjBlurParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_object_blur, px_grid(p.W, p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace shs_internal
