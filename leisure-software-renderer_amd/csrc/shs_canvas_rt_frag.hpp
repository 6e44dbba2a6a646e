// shs_canvas_rt_frag.hpp -- the fragment front end of the Canvas render-target raster's camera pass: what every
// fragment shader of shs_canvas_rt_shaders.hpp does before its own lighting, written once.  Included by
// shs_canvas_rt.hip alone (one translation unit; its header comment names the demos and their "soft :line" /
// "pbr :line" / "shafts :line" / "ibl :line" / "water :line" citations).
//   Frag            the shown fragment's record, varyings and draw, and the interpolations of the camera pass
//                   (:971-1013; soft :961-979; pbr :986-1035; ibl :810-852; water :2060-2211): world(), normal(), uv()
//   FragLinear      the same for the unclipped raster of hello_multi_pass.cpp ("multi :line"; the same text in
//                   hello_camera_and_perobject_motion_blur.cpp) and hello_glowing_star.cpp ("star :line"): no 1 / w
//   frag_velocity   the velocity of the fragment (:1002-1011; pbr :1017-1026; ibl :841-850; the water demo's is the
//                   hard demo's text)
//   frag_base01     the base colour in [0, 1]: the draw's, or sample_nearest of its texture
//   shadow_factor, pcss_from_world   the two shadow lookups from a world position
//   pack_rgba       three channels * 255 to the truncated bytes
// Every helper is text moved out of the shaders: the operands and the order of each float operation are theirs
// (the library is built without contraction, so a regrouped expression would round differently).
#pragma once
#include <float.h>
#include <limits.h>

#include "shs_canvas_rt_internal.hpp"
#include "shs_device.hpp"
#include "../../include/shs_gpu.h"

namespace shs_dev {
namespace {

// (int)f as the reference's x86-64 build converts it (cvttss2si: NaN and out-of-range give INT_MIN)
__device__ __forceinline__ int int_x86(float f) {
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// (int)std::lround(x) of a product that is NaN or lies in [0, n - 1] (as the legacy
// texture path's nearest_coord): halves away from zero; glibc's lroundf(NaN) is LONG_MIN, whose (int) is 0
__device__ __forceinline__ int lround_x86(float x) {
    if (!(x == x)) return 0;
    const float t = truncf(x);
    return (int)t + ((x - t >= 0.5f) ? 1 : 0);
}
__device__ __forceinline__ float pow64(float x) {
    double d = (double)x;
#pragma unroll
    for (int i = 0; i < 6; ++i) d = d * d;
    return (float)d;
}
__device__ __forceinline__ uint32_t byte_x86(float x) { return x == x ? (uint32_t)(int32_t)x & 0xffu : 0u; }
// rgb01_to_color up to the alpha: the three channels * 255, truncated as the x86-64 build truncates them
__device__ __forceinline__ uint32_t pack_rgba(float pr, float pg, float pb) {
    return byte_x86(pr) | (byte_x86(pg) << 8) | (byte_x86(pb) << 16) | 0xff000000u;
}
// color_to_rgb01 of a texel or canvas pixel (shs_renderer.hpp:291-293)
__device__ __forceinline__ f3 rgb01(uint32_t c) {
    return {(float)(c & 0xffu) / 255.0f, (float)((c >> 8) & 0xffu) / 255.0f, (float)((c >> 16) & 0xffu) / 255.0f};
}

__device__ __forceinline__ float saturate(float v) { return (v < 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v); }
__device__ __forceinline__ f3 mix3(f3 x, f3 y, float a) {   // glm::mix(x, y, a): x * (1 - a) + y * a
    const float b = 1.0f - a;
    return {x.x * b + y.x * a, x.y * b + y.y * a, x.z * b + y.z * a};
}
// glm::reflect(I, N) (detail/func_geometric.inl compute_reflect): I - N * dot(N, I) * 2, the vector scaled by the dot
// product and then by two
__device__ __forceinline__ f3 reflect3(f3 I, f3 N) {
    const float ni = dot3(N, I);
    return {I.x - N.x * ni * 2.0f, I.y - N.y * ni * 2.0f, I.z - N.z * ni * 2.0f};
}

// ---- the interpolations --------------------------------------------------------------------------------

// b0 * a0 + b1 * a1 + b2 * a2 as the reference's loops sum it: left to right
__device__ __forceinline__ float bary3(float u, float v, float w, float a0, float a1, float a2) { return (u * a0 + v * a1) + w * a2; }

// The shown fragment of a camera-pass pixel at the shading sub-triangle's barycentrics.  A shader calls what it
// reads: nothing is formed before it is asked for.
struct Frag {
    const RtRec &r;
    const RtVary &y;
    const RtDrawGPU &dr;
    float u, v, w;
    float iw0, iw1, iw2, invw_sum;

    __device__ __forceinline__ Frag(const RtParams &p, int32_t id, float u_, float v_, float w_)
        : r(p.recs[id]), y(p.vary[id]), dr(p.draws[p.recs[id].draw]), u(u_), v(v_), w(w_), iw0(r.iw0), iw1(r.iw1), iw2(r.iw2),
          invw_sum(bary3(u_, v_, w_, r.iw0, r.iw1, r.iw2)) {}

    // perspective-correct: the corners' values over w, summed, over the summed 1 / w
    __device__ __forceinline__ float persp(float a0, float a1, float a2) const {
        return bary3(u, v, w, a0 * iw0, a1 * iw1, a2 * iw2) / invw_sum;
    }
    __device__ __forceinline__ f3 world() const {
        return {persp(y.world[0], y.world[3], y.world[6]), persp(y.world[1], y.world[4], y.world[7]), persp(y.world[2], y.world[5], y.world[8])};
    }
    __device__ __forceinline__ float2 uv() const {
        return make_float2(persp(y.uv[0], y.uv[2], y.uv[4]), persp(y.uv[1], y.uv[3], y.uv[5]));
    }
    // the screen-linear normal: normalised by the raster and again by the fragment shader's first line
    __device__ __forceinline__ f3 normal() const {
        const f3 nsum = {bary3(u, v, w, y.nrm[0], y.nrm[3], y.nrm[6]), bary3(u, v, w, y.nrm[1], y.nrm[4], y.nrm[7]),
                         bary3(u, v, w, y.nrm[2], y.nrm[5], y.nrm[8])};
        return normalize3(normalize3(nsum));
    }
};

// The shown fragment of the unclipped raster (multi :575-581; star :407-413): every varying is interpolated
// screen-linearly, so the record's 1 / w terms are not read.
struct FragLinear {
    const RtVary &y;
    const RtDrawGPU &dr;
    float u, v, w;

    __device__ __forceinline__ FragLinear(const RtParams &p, int32_t id, float u_, float v_, float w_)
        : y(p.vary[id]), dr(p.draws[p.recs[id].draw]), u(u_), v(v_), w(w_) {}

    __device__ __forceinline__ f3 world() const {
        return {bary3(u, v, w, y.world[0], y.world[3], y.world[6]), bary3(u, v, w, y.world[1], y.world[4], y.world[7]),
                bary3(u, v, w, y.world[2], y.world[5], y.world[8])};
    }
    // normalised by the raster and again by the fragment shader's first line, as Frag::normal
    __device__ __forceinline__ f3 normal() const {
        const f3 nsum = {bary3(u, v, w, y.nrm[0], y.nrm[3], y.nrm[6]), bary3(u, v, w, y.nrm[1], y.nrm[4], y.nrm[7]),
                         bary3(u, v, w, y.nrm[2], y.nrm[5], y.nrm[8])};
        return normalize3(normalize3(nsum));
    }
};

// Canvas::clip_to_screen's x and y of an interpolated clip position
__device__ __forceinline__ void to_screen(const RtParams &p, float x, float y, float w, float &sx, float &sy) {
    const float nx = x / w, ny = y / w;
    sx = (nx + 1.0f) * 0.5f * (float)(p.W - 1);
    sy = (1.0f - ny) * 0.5f * (float)(p.H - 1);
}

// The velocity of the fragment: position and prev_position interpolated screen-linearly (their z is not read),
// both to the screen, the difference with y up, clamped to max_velocity in length.  min_len: the second threshold of
// the clamp, 1e-6f in the clipped demos and 0.0001f in the unclipped ones ("multi :589", "star :422").
__device__ __forceinline__ float2 frag_velocity(const RtParams &p, const RtVary &y, float u, float v, float w, float min_len = 1e-6f) {
    float csx, csy, psx, psy;
    to_screen(p, bary3(u, v, w, y.pos[0], y.pos[4], y.pos[8]), bary3(u, v, w, y.pos[1], y.pos[5], y.pos[9]),
              bary3(u, v, w, y.pos[3], y.pos[7], y.pos[11]), csx, csy);
    to_screen(p, bary3(u, v, w, y.prev[0], y.prev[4], y.prev[8]), bary3(u, v, w, y.prev[1], y.prev[5], y.prev[9]),
              bary3(u, v, w, y.prev[3], y.prev[7], y.prev[11]), psx, psy);
    float vx = csx - psx, vy = -(csy - psy);
    const float len = sqrtf(vx * vx + vy * vy);
    if (len > p.max_velocity && len > min_len) {
        const float s = p.max_velocity / len;
        vx *= s;
        vy *= s;
    }
    return make_float2(vx, vy);
}

// velocity_fragment_shader's velocity (hello_per_object_motion_blur.cpp:170-174), formed per pixel: the interpolated
// clip position and previous clip position (:436-437), each over its own interpolated w, the difference, * 0.5f, *
// viewport_size = (W, H).  +Y up as it stands; no clamp and no threshold, so a w of 0 stores the Inf or NaN it gives.
__device__ __forceinline__ float2 frag_velocity_ndc(const RtParams &p, const RtVary &y, float u, float v, float w) {
    const float cw = bary3(u, v, w, y.pos[3], y.pos[7], y.pos[11]);
    const float qw = bary3(u, v, w, y.prev[3], y.prev[7], y.prev[11]);
    const float cx = bary3(u, v, w, y.pos[0], y.pos[4], y.pos[8]) / cw, cy = bary3(u, v, w, y.pos[1], y.pos[5], y.pos[9]) / cw;
    const float qx = bary3(u, v, w, y.prev[0], y.prev[4], y.prev[8]) / qw, qy = bary3(u, v, w, y.prev[1], y.prev[5], y.prev[9]) / qw;
    return make_float2((cx - qx) * 0.5f * (float)p.W, (cy - qy) * 0.5f * (float)p.H);
}

// sample_nearest (shs_renderer.hpp:367-377; soft :167-186; water :121-140) up to the texel
__device__ __forceinline__ uint32_t sample_nearest_texel(const RtDrawGPU &dr, float tu, float tv) {
    const float su = saturate(tu), sv = saturate(tv);
    const int x = clampi(lround_x86(su * (float)(dr.tw - 1)), 0, dr.tw - 1);
    const int yy = clampi(lround_x86(sv * (float)(dr.th - 1)), 0, dr.th - 1);
    return dr.texels[(size_t)yy * dr.tw + x];
}

// The base colour of the Blinn-Phong shaders: color_to_rgb01 of the draw's colour, or of its texture at the fragment's
// uv, which is formed for a textured draw only
__device__ __forceinline__ f3 frag_base01(const Frag &f) {
    f3 base = {f.dr.colf[0] / 255.0f, f.dr.colf[1] / 255.0f, f.dr.colf[2] / 255.0f};
    if (f.dr.texels) {
        const float2 t = f.uv();
        base = rgb01(sample_nearest_texel(f.dr, t.x, t.y));
    }
    return base;
}

// ---- the shadow lookups from a world position ------------------------------------------------------------

__device__ __forceinline__ float sm_sample(const RtParams &p, int x, int y) {   // ShadowMap::sample :637-640
    if (x < 0 || x >= p.sw || y < 0 || y >= p.sh) return FLT_MAX;
    return p.shadow[(size_t)y * p.sw + x];
}

// shadow_uvz_from_world, shadow_compare / shadow_factor_pcf_2x2 (:628-693) as fragment_shader_full calls them
__device__ float shadow_factor(const RtParams &p, f3 wp, float ndotl) {
    float cx, cy, cz, cw;
    m4p(p.light_vp, wp.x, wp.y, wp.z, cx, cy, cz, cw);
    if (fabsf(cw) < 1e-6f) return 1.0f;
    const float nx = cx / cw, ny = cy / cw, z = cz / cw;
    if (z < 0.0f || z > 1.0f) return 1.0f;
    const float u = nx * 0.5f + 0.5f;
    const float v = 1.0f - (ny * 0.5f + 0.5f);
    const float slope = 1.0f - g_clamp01(ndotl);
    const float bias = p.bias_base + p.bias_slope * slope;
    if (!(p.flags & SHS_RT_PCF)) {
        if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) return 1.0f;
        const int x = lround_x86(u * (float)(p.sw - 1));
        const int y = lround_x86(v * (float)(p.sh - 1));
        const float d = sm_sample(p, x, y);
        if (d == FLT_MAX) return 1.0f;
        return (z <= d + bias) ? 1.0f : 0.0f;
    }
    const float fx = u * (float)(p.sw - 1);
    const float fy = v * (float)(p.sh - 1);
    const int x0 = clampi(int_x86(floorf(fx)), 0, p.sw - 1);
    const int y0 = clampi(int_x86(floorf(fy)), 0, p.sh - 1);
    const int x1 = clampi(x0 + 1, 0, p.sw - 1);
    const int y1 = clampi(y0 + 1, 0, p.sh - 1);
    const float s00 = (z <= sm_sample(p, x0, y0) + bias) ? 1.0f : 0.0f;
    const float s10 = (z <= sm_sample(p, x1, y0) + bias) ? 1.0f : 0.0f;
    const float s01 = (z <= sm_sample(p, x0, y1) + bias) ? 1.0f : 0.0f;
    const float s11 = (z <= sm_sample(p, x1, y1) + bias) ? 1.0f : 0.0f;
    return 0.25f * (((s00 + s10) + s01) + s11);
}

// POISSON_32 (soft :267-301); a tap's index is wave-uniform, so these are scalar loads
__constant__ float2 c_poisson32[32] = {
    {-0.613392f, 0.617481f},  {0.170019f, -0.040254f},  {-0.299417f, 0.791925f},  {0.645680f, 0.493210f},
    {-0.651784f, 0.717887f},  {0.421003f, 0.027070f},   {-0.817194f, -0.271096f}, {-0.705374f, -0.668203f},
    {0.977050f, -0.108615f},  {0.063326f, 0.142369f},   {0.203528f, 0.214331f},   {-0.667531f, 0.326090f},
    {-0.098422f, -0.295755f}, {-0.885922f, 0.215369f},  {0.566637f, 0.605213f},   {0.039766f, -0.396100f},
    {0.751946f, 0.453352f},   {0.078707f, -0.715323f},  {-0.075838f, -0.529344f}, {0.724479f, -0.580798f},
    {0.222999f, -0.215125f},  {-0.467574f, -0.405438f}, {-0.248268f, -0.814753f}, {0.354411f, -0.887570f},
    {0.175817f, 0.382366f},   {0.487472f, -0.063082f},  {-0.084078f, 0.898312f},  {0.488876f, -0.783441f},
    {0.470016f, 0.217933f},   {-0.696890f, -0.549791f}, {-0.149693f, 0.605762f},  {0.034211f, 0.979980f}};

struct PcssMap {   // the soft demo's file-local ShadowMap (:191-225) and the constants of shs_rt_pcss
    const float *depth;
    int w, h;
    float light, search, fmin, fmax, eps;
    int blockers, taps;
};
// c: RtParams or RtPcssSamples, which hold the seven constants under the same names
template <class Consts>
__device__ __forceinline__ PcssMap pcss_map(const float *depth, int w, int h, const Consts &c) {
    return {depth, w, h, c.pcss_light, c.pcss_search, c.pcss_min, c.pcss_max, c.pcss_eps, c.pcss_blockers, c.pcss_taps};
}

// shadow_sample_depth_uv (soft :252-261) over ShadowMap::sample (:219-224), which clamps: a uv outside [0, 1]
// is FLT_MAX (empty) without a read; a NaN passes the range test and reads texel 0 of its axis.  The load is
// unconditional at a clamped address, so the taps of a loop are independent gathers the compiler may batch.
__device__ __forceinline__ float pcss_tap(const PcssMap &m, float u, float v) {
    const bool off = u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f;
    const int x = clampi(lround_x86(u * (float)(m.w - 1)), 0, m.w - 1);
    const int y = clampi(lround_x86(v * (float)(m.h - 1)), 0, m.h - 1);
    const float d = m.depth[(size_t)y * m.w + x];
    return off ? FLT_MAX : d;
}

// pcss_shadow_factor (soft :333-445; shafts :650-762).  rot: {cos(ang), sin(ang), cos(ang2), sin(ang2)} of the screen
// pixel, the host libm's values; rotate2's multiplies and add / subtract run here.
__device__ float pcss_shadow_factor(const PcssMap &m, float u, float v, float z, float bias, float4 rot) {
    if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) return 1.0f;
    if (pcss_tap(m, u, v) == FLT_MAX) return 1.0f;
    const float tsu = 1.0f / (float)m.w, tsv = 1.0f / (float)m.h;
    const float sru = m.search * tsu, srv = m.search * tsv;
    const float ztest = z - bias;
    float bsum = 0.0f;
    int bcnt = 0;
#pragma unroll 4
    for (int i = 0; i < m.blockers; ++i) {
        const float2 o = c_poisson32[i & 31];
        const float ox = rot.x * o.x - rot.y * o.y, oy = rot.y * o.x + rot.x * o.y;
        const float d = pcss_tap(m, u + ox * sru, v + oy * srv);
        const bool blocks = d != FLT_MAX && d < ztest;
        bsum = blocks ? bsum + d : bsum;
        bcnt += blocks ? 1 : 0;
    }
    if (bcnt <= 0) return 1.0f;
    const float avg = bsum / (float)bcnt;
    const float zb = g_max(m.eps, avg), zr = g_max(m.eps, z);   // std::max(a, b): (a < b) ? b : a
    const float ratio = g_max(0.0f, (zr - zb) / zb);
    const float fuu = m.light * ratio, fuv = m.light * ratio;
    float ft = 0.5f * (fuu / tsu + fuv / tsv);
    ft = (ft < m.fmin) ? m.fmin : (ft > m.fmax ? m.fmax : ft);  // clampf :127-132
    const float fru = ft * tsu, frv = ft * tsv;
    if (m.taps <= 0) return 1.0f;
    float lit = 0.0f;
#pragma unroll 4
    for (int i = 0; i < m.taps; ++i) {
        const float2 o = c_poisson32[i & 31];
        const float ox = rot.z * o.x - rot.w * o.y, oy = rot.w * o.x + rot.z * o.y;
        const float d = pcss_tap(m, u + ox * fru, v + oy * frv);
        lit += (d == FLT_MAX || z <= d + bias) ? 1.0f : 0.0f;   // empty and off-map taps count as lit
    }
    return lit / (float)m.taps;
}

// shadow_uvz_from_world (soft :231-250; shafts :558-576), the slope-scaled bias (shafts :814-815, the soft shader's
// text) and pcss_shadow_factor at screen pixel (px, py) over the bound map; lit where the lookup leaves the light's
// clip volume
__device__ __forceinline__ float pcss_from_world(const RtParams &p, f3 wp, float ndotl, int px, int py) {
    float shadow = 1.0f;
    float cx, cy, cz, cw;
    m4p(p.light_vp, wp.x, wp.y, wp.z, cx, cy, cz, cw);
    if (!(fabsf(cw) < 1e-6f)) {
        const float nx = cx / cw, ny = cy / cw, z = cz / cw;
        if (!(z < 0.0f || z > 1.0f)) {
            const float su = nx * 0.5f + 0.5f;
            const float sv = 1.0f - (ny * 0.5f + 0.5f);
            const float slope = 1.0f - g_clamp01(ndotl);
            const float bias = p.bias_base + p.bias_slope * slope;
            shadow = pcss_shadow_factor(pcss_map(p.shadow, p.sw, p.sh, p), su, sv, z, bias, p.rot[(size_t)py * p.W + px]);
        }
    }
    return shadow;
}

}  // namespace
}  // namespace shs_dev
