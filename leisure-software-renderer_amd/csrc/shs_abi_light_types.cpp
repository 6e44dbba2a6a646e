// shs_abi_light_types.cpp -- host side of the typed local lights (include/shs_gpu.h, "typed local
// lights"): ILightModel::pack_for_culling of the four light models and the per-light shading
// constants of SHS_PROGRAM_FORWARD_PLUS_TYPED.  Everything here restates the reference's own float
// expressions in its operation order (no FMA contraction); paths are relative to the reference's
// cpp-folders/src/shs-renderer-lib/include/shs/.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/shs_gpu.h"
#include "shs_ctx.hpp"
#include "shs_glm.hpp"
#include "shs_lib_device.hpp"

using namespace shs_host;

static_assert(sizeof(shs_light_props) == 128, "shs_light_props is 128 B");

namespace {

constexpr float HALF_PI = 1.57079632679489661923132169163975144f;   // glm::half_pi<float>()

inline vec3 v3(const float *p) { return {p[0], p[1], p[2]}; }
inline void put(float *o, vec3 v, float w) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = w; }
inline float len3(vec3 v) { return std::sqrt(gdot(v, v)); }   // glm::length
inline vec3 gmax0(vec3 v) { return {std::max(v.x, 0.0f), std::max(v.y, 0.0f), std::max(v.z, 0.0f)}; }
inline vec3 gabs(vec3 v) { return {std::fabs(v.x), std::fabs(v.y), std::fabs(v.z)}; }

// normalize_or (geometry/volumes.hpp:135-140)
inline vec3 normalize_or(vec3 v, vec3 fallback) {
    const float len2 = gdot(v, v);
    if (len2 <= 1e-10f) return fallback;
    return gscale(v, 1.0f / std::sqrt(len2));
}

// safe_forward (lighting/light_runtime.hpp:133-136)
inline vec3 safe_forward(const shs_light_props &p) { return normalize_or(v3(p.direction_ws), vec3{0.0f, -1.0f, 0.0f}); }

// basis_from_forward_and_hint (light_runtime.hpp:138-151); right_from_forward (camera/camera_math.hpp
// :28-31) is evaluated before normalize_or looks at its first argument, as a C++ argument is
inline void basis_from_forward_and_hint(vec3 forward, vec3 up_hint, vec3 &right, vec3 &up, vec3 &fwd) {
    fwd = normalize_or(forward, vec3{0.0f, 0.0f, 1.0f});
    const vec3 up_ref = normalize_or(up_hint, vec3{0.0f, 1.0f, 0.0f});
    right = gcross(up_ref, fwd);
    right = normalize_or(right, gnormalize(gcross(up_ref, fwd)));
    up = normalize_or(gcross(fwd, right), vec3{0.0f, 1.0f, 0.0f});
    right = normalize_or(gcross(up, fwd), right);
}

inline bool finite3(vec3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }

// make_light_common (light_runtime.hpp:167-180)
struct Common {
    vec3 position, color;
    float range, intensity, power, bias, cutoff;
    uint32_t flags, model;
};
inline Common make_light_common(const shs_light_props &p) {
    Common c;
    c.position = v3(p.position_ws);
    c.range = std::max(p.range, 0.001f);
    c.color = gmax0(v3(p.color));
    c.intensity = std::max(p.intensity, 0.0f);
    c.flags = p.flags;
    c.model = p.attenuation_model;
    c.power = std::max(p.attenuation_power, 0.001f);
    c.bias = std::max(p.attenuation_bias, 1e-5f);
    c.cutoff = std::max(p.attenuation_cutoff, 0.0f);
    return c;
}

// The fields every make_*_culling_light writes alike (lighting/light_types.hpp:327-435) and
// assign_light_cull_bounds (:203-212).
void pack_common(const Common &c, uint32_t type, uint32_t shape, float shape_y, vec3 sphere_c, float sphere_r, vec3 amin,
                 vec3 amax, shs_culling_light &o) {
    put(o.position_range, c.position, std::max(c.range, 0.0f));
    put(o.color_intensity, gmax0(c.color), std::max(c.intensity, 0.0f));
    o.shape_attenuation[0] = shape_y;
    o.shape_attenuation[1] = std::max(c.power, 0.001f);
    o.shape_attenuation[2] = std::max(c.bias, 1e-5f);
    o.shape_attenuation[3] = std::max(c.cutoff, 0.0f);
    o.type_shape_flags[0] = type; o.type_shape_flags[1] = shape; o.type_shape_flags[2] = c.flags; o.type_shape_flags[3] = c.model;
    put(o.cull_sphere, sphere_c, std::max(sphere_r, 0.0f));
    put(o.cull_aabb_min, amin, 1.0f);
    put(o.cull_aabb_max, amax, 1.0f);
}

// aabb_from_sphere (light_types.hpp:169-177)
inline void aabb_from_sphere(vec3 c, float radius, vec3 &mn, vec3 &mx) {
    const float r = std::max(radius, 0.0f);
    mn = gsub(c, vec3{r, r, r});
    mx = gadd(c, vec3{r, r, r});
}

// PointLightModel::pack_for_culling (light_runtime.hpp:309-314) -> make_point_culling_light
void pack_point(const shs_light_props &p, shs_culling_light &o) {
    const Common c = make_light_common(p);
    const float r = std::max(c.range, 0.0f);   // point_light_culling_sphere (light_types.hpp:251-257)
    vec3 mn, mx;
    aabb_from_sphere(c.position, r, mn, mx);
    put(o.direction_spot, vec3{0.0f, -1.0f, 0.0f}, 1.0f);
    put(o.axis_spot_outer, vec3{1.0f, 0.0f, 0.0f}, 0.0f);
    put(o.up_shape_x, vec3{0.0f, 1.0f, 0.0f}, 0.0f);
    pack_common(c, 1u, 1u, 0.0f, c.position, r, mn, mx, o);   // Point, Sphere
}

// SpotLightModel::pack_for_culling (light_runtime.hpp:357-367) -> make_spot_culling_light (:351-379)
void pack_spot(const shs_light_props &p, shs_culling_light &o) {
    const Common c = make_light_common(p);
    const vec3 sdir = safe_forward(p);
    const float sinner = std::clamp(p.inner_angle_rad, 0.02f, HALF_PI - 0.02f);
    const float souter = std::clamp(std::max(sinner + 0.005f, p.outer_angle_rad), sinner + 0.005f, HALF_PI - 0.005f);
    const float r = std::max(c.range, 0.0f);   // spot_light_culling_sphere
    const vec3 dir = normalize_or(sdir, vec3{0.0f, -1.0f, 0.0f});
    const float inner = std::clamp(sinner, 0.01f, HALF_PI - 0.01f);
    const float outer = std::clamp(std::max(inner + 0.001f, souter), inner + 0.001f, HALF_PI - 0.001f);
    vec3 mn, mx;
    aabb_from_sphere(c.position, r, mn, mx);
    put(o.direction_spot, dir, std::cos(inner));
    put(o.axis_spot_outer, vec3{1.0f, 0.0f, 0.0f}, std::cos(outer));
    put(o.up_shape_x, vec3{0.0f, 1.0f, 0.0f}, 0.0f);
    pack_common(c, 2u, 2u, 0.0f, c.position, r, mn, mx, o);   // Spot, Cone
}

// RectAreaLightModel::pack_for_culling (light_runtime.hpp:425-436) -> make_rect_area_culling_light
// (light_types.hpp:381-406) over rect_area_light_culling_obb / _sphere (:267-299), aabb_from_obb (:179-191)
void pack_rect(const shs_light_props &p, shs_culling_light &o) {
    vec3 bright, bup, bfwd;
    basis_from_forward_and_hint(safe_forward(p), v3(p.up_ws), bright, bup, bfwd);
    const Common c = make_light_common(p);
    const float ex = std::max(p.rect_half_extents[0], 0.1f), ey = std::max(p.rect_half_extents[1], 0.1f);
    const vec3 dir = normalize_or(bfwd, vec3{0.0f, -1.0f, 0.0f});
    vec3 right = gsub(bright, gscale(dir, gdot(bright, dir)));
    right = normalize_or(right, vec3{1.0f, 0.0f, 0.0f});
    const vec3 up = gnormalize(gcross(dir, right));
    right = normalize_or(gcross(up, dir), right);
    const float hx = std::max(ex, 0.001f), hy = std::max(ey, 0.001f);
    const float range = std::max(c.range, 0.0f);
    const vec3 center = gadd(c.position, gscale(dir, range * 0.5f));
    const vec3 he = {hx + range, hy + range, std::max(range * 0.5f, 0.001f)};
    const vec3 e0 = gmax0(he);
    const vec3 wext = gadd(gadd(gscale(gabs(right), e0.x), gscale(gabs(up), e0.y)), gscale(gabs(dir), e0.z));
    put(o.direction_spot, gneg(dir), 1.0f);
    put(o.axis_spot_outer, right, 0.0f);
    put(o.up_shape_x, up, he.x);
    pack_common(c, 3u, 3u, he.y, center, len3(he), gsub(center, wext), gadd(center, wext), o);   // RectArea, OrientedBox
}

// TubeAreaLightModel::pack_for_culling (light_runtime.hpp:494-502) -> make_tube_area_culling_light
// (light_types.hpp:408-435) over tube_area_light_culling_capsule / _sphere (:301-324), aabb_from_capsule (:193-201)
void pack_tube(const shs_light_props &p, shs_culling_light &o) {
    const Common c = make_light_common(p);
    const vec3 taxis = normalize_or(v3(p.right_ws), vec3{1.0f, 0.0f, 0.0f});
    const float thalf = std::max(p.tube_half_length, 0.1f), tradius = std::max(p.tube_radius, 0.05f);
    const vec3 axis0 = normalize_or(taxis, vec3{1.0f, 0.0f, 0.0f});
    const float half_len = std::max(thalf, 0.001f);
    const float radius = std::max(std::max(c.range, 0.0f), std::max(tradius, 0.001f));
    const vec3 a = gsub(c.position, gscale(axis0, half_len)), b = gadd(c.position, gscale(axis0, half_len));
    const vec3 ab = gsub(b, a);
    const float sphere_r = std::max(len3(ab) * 0.5f + radius, 0.0f);
    const vec3 axis = normalize_or(ab, vec3{1.0f, 0.0f, 0.0f});
    const float r = std::max(radius, 0.0f);
    const vec3 lo = {std::min(a.x, b.x), std::min(a.y, b.y), std::min(a.z, b.z)};
    const vec3 hi = {std::max(a.x, b.x), std::max(a.y, b.y), std::max(a.z, b.z)};
    put(o.direction_spot, axis, 1.0f);
    put(o.axis_spot_outer, axis, 0.0f);
    put(o.up_shape_x, vec3{0.0f, 1.0f, 0.0f}, len3(ab) * 0.5f);
    pack_common(c, 4u, 4u, radius, c.position, sphere_r, gsub(lo, vec3{r, r, r}), gadd(hi, vec3{r, r, r}), o);   // TubeArea, Capsule
}

// A float not below the double x (the wave cull's bounding radii are rounded up).
inline float round_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    return f;
}

// The shading record of one light: what its sample function (light_runtime.hpp:321-333, 376-402,
// 445-471, 514-534) computes from the properties alone.  False: the rect basis is not finite.
bool shading_record(const shs_light_props &p, shs_dev::TLight &t) {
    std::memset(&t, 0, sizeof t);
    put(t.pos_range, v3(p.position_ws), p.range);
    put(t.color_int, v3(p.color), p.intensity);
    t.atten[0] = p.attenuation_power; t.atten[1] = p.attenuation_bias; t.atten[2] = p.attenuation_cutoff;
    std::memcpy(&t.atten[3], &p.attenuation_model, sizeof(uint32_t));
    std::memcpy(&t.shape[0], &p.type, sizeof(uint32_t));
    // Bounding sphere around position_ws outside which the light adds exactly nothing (k_lib_resolve's
    // wave cull, cull_wave_list): the emitting point lies within `extent` of the position.
    double extent = 0.0;
    if (p.type == SHS_LIGHT_SPOT) {
        put(t.v0, safe_forward(p), 0.0f);
        const float inner = std::clamp(p.inner_angle_rad, 0.02f, HALF_PI - 0.02f);
        const float outer = std::clamp(std::max(inner + 0.005f, p.outer_angle_rad), inner + 0.005f, HALF_PI - 0.005f);
        const float cos_inner = std::cos(inner), cos_outer = std::cos(outer);
        t.shape[2] = cos_outer;
        t.shape[3] = std::max(cos_inner - cos_outer, 1e-5f);
    } else if (p.type == SHS_LIGHT_RECT_AREA) {
        vec3 right, up, fwd;
        basis_from_forward_and_hint(safe_forward(p), v3(p.up_ws), right, up, fwd);
        if (!finite3(right) || !finite3(up) || !finite3(fwd)) return false;
        const float hx = std::max(p.rect_half_extents[0], 0.05f), hy = std::max(p.rect_half_extents[1], 0.05f);
        put(t.v0, fwd, hx);
        put(t.v1, right, hy);
        put(t.v2, up, 0.0f);
        extent = std::sqrt((double)hx * hx + (double)hy * hy);
    } else if (p.type == SHS_LIGHT_TUBE_AREA) {
        const vec3 axis = normalize_or(v3(p.right_ws), vec3{1.0f, 0.0f, 0.0f});
        const float half_len = std::max(p.tube_half_length, 0.1f);
        const vec3 pos = v3(p.position_ws);
        const vec3 a = gsub(pos, gscale(axis, half_len)), b = gadd(pos, gscale(axis, half_len));
        const vec3 ab = gsub(b, a);   // closest_point_on_segment (:254-261)
        put(t.v0, a, gdot(ab, ab));
        put(t.v1, ab, 0.0f);
        extent = half_len;
    }
    // (extent + range) widened by 2^-10, plus the rounding of the emitting point's own coordinates (a
    // few roundings of 2^-24 relative to |position| + extent; 2^-18 of their sum covers them)
    const double mag = std::fabs((double)p.position_ws[0]) + std::fabs((double)p.position_ws[1]) + std::fabs((double)p.position_ws[2]);
    t.shape[1] = round_up((extent + std::max((double)p.range, 0.0)) * (1.0 + 0x1p-10) + (mag + extent) * 0x1p-18);
    return true;
}

}  // namespace

extern "C" {

int shs_light_pack_culling(const shs_light_props *props, int32_t n, shs_culling_light *out) {
    if (n < 0 || (n > 0 && (!props || !out))) return SHS_ERR_INVALID;
    for (int32_t i = 0; i < n; ++i) {
        shs_culling_light o;
        std::memset(&o, 0, sizeof o);
        switch (props[i].type) {
            case SHS_LIGHT_POINT: pack_point(props[i], o); break;
            case SHS_LIGHT_SPOT: pack_spot(props[i], o); break;
            case SHS_LIGHT_RECT_AREA: pack_rect(props[i], o); break;
            case SHS_LIGHT_TUBE_AREA: pack_tube(props[i], o); break;
            default: return SHS_ERR_INVALID;
        }
        out[i] = o;
    }
    return SHS_OK;
}

int shs_lights_upload_typed(shs_ctx *ctx, const shs_culling_light *cull, const shs_light_props *props, int32_t n) {
    if (!ctx || n < 0 || (n > 0 && (!cull || !props))) return SHS_ERR_INVALID;
    std::vector<shs_dev::TLight> rec((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        if (props[i].type < SHS_LIGHT_POINT || props[i].type > SHS_LIGHT_TUBE_AREA) {
            ctx->err = "light " + std::to_string(i) + ": type " + std::to_string(props[i].type) + " is not a local light type (1-4)";
            return SHS_ERR_INVALID;
        }
        if (!shading_record(props[i], rec[(size_t)i])) {
            ctx->err = "light " + std::to_string(i) + ": rect-area light with up_ws parallel to its forward direction (no basis)";
            return SHS_ERR_INVALID;
        }
    }
    const int rc = shs_lights_upload(ctx, cull, n);   // (also marks the set untyped and the lists stale)
    if (rc) return rc;
    if (ensure(ctx, ctx->tlights, (size_t)std::max(n, 1))) return SHS_ERR_HIP;
    if (n > 0) HIP_TRY(ctx, hipMemcpy(ctx->tlights.p, rec.data(), (size_t)n * sizeof(shs_dev::TLight), hipMemcpyHostToDevice));
    ctx->lights_typed = true;
    return SHS_OK;
}

}  // extern "C"
