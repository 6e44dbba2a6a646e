/*
 * ref_light_models.c -- TEST INFRASTRUCTURE ONLY: C restatement of the four ILightModel::sample
 * functions of shs-renderer-lib (include/shs/lighting/light_runtime.hpp) for the typed Forward+ tests.
 *   normalize_or                     geometry/volumes.hpp:135-140
 *   right_from_forward               camera/camera_math.hpp:28-31
 *   safe_forward                     lighting/light_runtime.hpp:133-136
 *   basis_from_forward_and_hint      :138-151
 *   eval_distance_attenuation        :182-210
 *   eval_local_light_brdf            :212-237
 *   closest_point_on_segment         :254-261
 *   PointLightModel::sample          :321-333
 *   SpotLightModel::sample           :376-402
 *   RectAreaLightModel::sample       :445-471
 *   TubeAreaLightModel::sample       :514-534
 * Every sample recomputes everything from the LightProperties, as the reference does.  GLM
 * operations in GLM's order (dot = (x + y) + z, normalize = v * (1 / sqrt(dot)), cross as
 * glm::cross), std::max / min / clamp as their comparisons; built without FMA contraction.
 *
 * libshs_light_types_ref.so links this file with the frozen oracle, whose rasteriser object is
 * compiled with -Dora_point_light_accumulate=ref_typed_light_accumulate: oracle.forward_plus then
 * evaluates every listed light through ref_typed_light_accumulate below, which finds the light's
 * properties by the record's index in the registered table.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/shs_gpu.h"
#include "../../oracle/shs_oracle.h"

typedef struct { float x, y, z; } v3;

static inline float fmaxs(float a, float b) { return (a < b) ? b : a; }   /* std::max */
static inline float fmins(float a, float b) { return (b < a) ? b : a; }   /* std::min */
static inline float fclamps(float v, float lo, float hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }   /* std::clamp */
static inline v3 mk(const float *p) { v3 r = {p[0], p[1], p[2]}; return r; }
static inline v3 add(v3 a, v3 b) { v3 r = {a.x + b.x, a.y + b.y, a.z + b.z}; return r; }
static inline v3 sub(v3 a, v3 b) { v3 r = {a.x - b.x, a.y - b.y, a.z - b.z}; return r; }
static inline v3 scl(v3 a, float s) { v3 r = {a.x * s, a.y * s, a.z * s}; return r; }
static inline v3 divs(v3 a, float s) { v3 r = {a.x / s, a.y / s, a.z / s}; return r; }
static inline v3 neg(v3 a) { v3 r = {-a.x, -a.y, -a.z}; return r; }
static inline float dot(v3 a, v3 b) { const float x = a.x * b.x, y = a.y * b.y, z = a.z * b.z; return (x + y) + z; }
static inline v3 cross(v3 x, v3 y) { v3 r = {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y}; return r; }
static inline float length(v3 a) { return sqrtf(dot(a, a)); }
static inline v3 normalize(v3 v) { return scl(v, 1.0f / sqrtf(dot(v, v))); }

static inline v3 normalize_or(v3 v, v3 fallback) {
    const float len2 = dot(v, v);
    if (len2 <= 1e-10f) return fallback;
    return scl(v, 1.0f / sqrtf(len2));
}

static v3 safe_forward(const shs_light_props *p) {
    const v3 down = {0.0f, -1.0f, 0.0f};
    return normalize_or(mk(p->direction_ws), down);
}

static void basis_from_forward_and_hint(v3 forward, v3 up_hint, v3 *out_right, v3 *out_up, v3 *out_forward) {
    const v3 z = {0.0f, 0.0f, 1.0f}, y = {0.0f, 1.0f, 0.0f};
    *out_forward = normalize_or(forward, z);
    const v3 up_ref = normalize_or(up_hint, y);
    *out_right = cross(up_ref, *out_forward);
    *out_right = normalize_or(*out_right, normalize(cross(up_ref, *out_forward)));   /* right_from_forward */
    *out_up = normalize_or(cross(*out_forward, *out_right), y);
    *out_right = normalize_or(cross(*out_up, *out_forward), *out_right);
}

static float eval_distance_attenuation(const shs_light_props *p, float distance) {
    const float range = fmaxs(p->range, 0.001f);
    if (distance >= range) return 0.0f;
    const float norm = fclamps(1.0f - distance / range, 0.0f, 1.0f);
    float falloff = 0.0f;
    switch (p->attenuation_model) {
        case 0u: falloff = norm; break;
        case 1u: falloff = norm * norm * (3.0f - 2.0f * norm); break;
        case 2u: {
            const float denom = fmaxs(distance * distance, p->attenuation_bias);
            const float inv = 1.0f / denom;
            const float range_norm = range * range;
            falloff = fmins(1.0f, inv * range_norm) * (norm * norm);
            break;
        }
        default: break;
    }
    falloff = powf(fmaxs(falloff, 0.0f), fmaxs(p->attenuation_power, 0.001f));
    if (p->attenuation_cutoff > 0.0f && falloff < p->attenuation_cutoff) return 0.0f;
    return fmaxs(falloff, 0.0f);
}

/* out6: LightContribution diffuse, specular (zero unless written) */
static void eval_local_light_brdf(const shs_light_props *p, v3 L, float distance, float shaping, float spec_power,
                                  float spec_scale, v3 n, v3 view, float *out6) {
    const float ndotl = fmaxs(dot(n, L), 0.0f);
    if (ndotl <= 0.0f) return;
    const float attenuation = eval_distance_attenuation(p, distance) * fmaxs(shaping, 0.0f);
    if (attenuation <= 0.0f) return;
    const float in = fmaxs(p->intensity, 0.0f);
    const v3 radiance = {fmaxs(p->color[0], 0.0f) * in * attenuation, fmaxs(p->color[1], 0.0f) * in * attenuation,
                         fmaxs(p->color[2], 0.0f) * in * attenuation};
    const v3 H = normalize_or(add(L, view), L);
    const float ndoth = fmaxs(dot(n, H), 0.0f);
    const float spec = (ndotl > 0.0f) ? (spec_scale * powf(ndoth, spec_power)) : 0.0f;
    out6[0] = radiance.x * ndotl; out6[1] = radiance.y * ndotl; out6[2] = radiance.z * ndotl;
    out6[3] = radiance.x * spec; out6[4] = radiance.y * spec; out6[5] = radiance.z * spec;
}

static v3 closest_point_on_segment(v3 p, v3 a, v3 b) {
    const v3 ab = sub(b, a);
    const float denom = dot(ab, ab);
    if (denom <= 1e-8f) return a;
    const float t = fclamps(dot(sub(p, a), ab) / denom, 0.0f, 1.0f);
    return add(a, scl(ab, t));
}

static const float HALF_PI = 1.57079632679489661923132169163975144f;   /* glm::half_pi<float>() */

/* ILightModel::sample of props->type -> out6 = (diffuse, specular) */
void ref_light_sample(const shs_light_props *p, const float *world_pos, const float *world_normal, const float *view_dir,
                      float *out6) {
    for (int k = 0; k < 6; ++k) out6[k] = 0.0f;
    const v3 world = mk(world_pos), n = mk(world_normal), view = mk(view_dir), pos = mk(p->position_ws);
    if (p->type == 1u) {
        const v3 to_light = sub(pos, world);
        const float dist = length(to_light);
        if (dist <= 1e-4f || dist > p->range) return;
        const v3 L = divs(to_light, dist);
        eval_local_light_brdf(p, L, dist, 1.0f, 36.0f, 0.30f, n, view, out6);
    } else if (p->type == 2u) {
        const v3 to_light = sub(pos, world);
        const float dist = length(to_light);
        if (dist <= 1e-4f || dist > p->range) return;
        const v3 L = divs(to_light, dist);
        const v3 light_to_surface = neg(L);
        const v3 dir = safe_forward(p);
        const float inner = fclamps(p->inner_angle_rad, 0.02f, HALF_PI - 0.02f);
        const float outer = fclamps(fmaxs(inner + 0.005f, p->outer_angle_rad), inner + 0.005f, HALF_PI - 0.005f);
        const float cos_inner = cosf(inner);
        const float cos_outer = cosf(outer);
        const float cos_theta = dot(light_to_surface, dir);
        if (cos_theta <= cos_outer) return;
        float t = (cos_theta - cos_outer) / fmaxs(cos_inner - cos_outer, 1e-5f);
        t = fclamps(t, 0.0f, 1.0f);
        const float shaping = t * t * (3.0f - 2.0f * t);
        eval_local_light_brdf(p, L, dist, shaping, 34.0f, 0.32f, n, view, out6);
    } else if (p->type == 3u) {
        v3 right, up, fwd;
        basis_from_forward_and_hint(safe_forward(p), mk(p->up_ws), &right, &up, &fwd);
        const float hx = fmaxs(p->rect_half_extents[0], 0.05f), hy = fmaxs(p->rect_half_extents[1], 0.05f);
        const v3 d = sub(world, pos);
        const float ux = fclamps(dot(d, right), -hx, hx);
        const float uy = fclamps(dot(d, up), -hy, hy);
        const v3 emit_pt = add(add(pos, scl(right, ux)), scl(up, uy));
        const v3 to_light = sub(emit_pt, world);
        const float dist = length(to_light);
        if (dist <= 1e-4f || dist > p->range) return;
        const v3 L = divs(to_light, dist);
        const v3 light_to_surface = neg(L);
        const float emission_facing = fmaxs(dot(fwd, light_to_surface), 0.0f);
        if (emission_facing <= 0.0f) return;
        const float shape_gain = 0.65f + 0.55f * emission_facing;
        eval_local_light_brdf(p, L, dist, shape_gain, 26.0f, 0.26f, n, view, out6);
    } else if (p->type == 4u) {
        const v3 x = {1.0f, 0.0f, 0.0f};
        const v3 axis = normalize_or(mk(p->right_ws), x);
        const float half_len = fmaxs(p->tube_half_length, 0.1f);
        const v3 a = sub(pos, scl(axis, half_len));
        const v3 b = add(pos, scl(axis, half_len));
        const v3 emit_pt = closest_point_on_segment(world, a, b);
        const v3 to_light = sub(emit_pt, world);
        const float dist = length(to_light);
        if (dist <= 1e-4f || dist > p->range) return;
        const v3 L = divs(to_light, dist);
        const float radial_softening = fclamps(1.0f - dist / fmaxs(p->range, 0.1f), 0.0f, 1.0f);
        const float shaping = 0.75f + 0.35f * radial_softening;
        eval_local_light_brdf(p, L, dist, shaping, 22.0f, 0.20f, n, view, out6);
    }
}

/* the properties of the light set oracle.forward_plus runs over: record i of `base` has props[i] */
static const ora_culling_light *g_base = NULL;
static const shs_light_props *g_props = NULL;
static int g_n = 0;
static volatile int g_misses = 0;   /* accumulate calls with a record outside the table (the tests assert 0) */

void ref_set_light_props(const void *base, const shs_light_props *props, int n) {
    g_base = (const ora_culling_light *)base;
    g_props = props;
    g_n = n;
    g_misses = 0;
}

int ref_light_misses(void) { return g_misses; }

/* include/shs_gpu.h's record sizes as a C compiler sees them (the ABI test compares _abi.py's) */
int ref_sizeof(int which) { return which == 0 ? (int)sizeof(shs_light_props) : (int)sizeof(shs_culling_light); }

/* Replaces ora_point_light_accumulate in the rasteriser object: lit += base * diffuse + specular
 * (exp-plumbing/hello_light_types_culling_sw.cpp:414).  A record outside the table adds nothing and is
 * reported by ref_light_misses. */
void ref_typed_light_accumulate(const ora_culling_light *L, const float *world, const float *N, const float *V,
                                const float *base, float *lit) {
    const ptrdiff_t idx = L - g_base;
    if (!g_props || idx < 0 || idx >= (ptrdiff_t)g_n) { g_misses = 1; return; }
    float c[6];
    ref_light_sample(&g_props[idx], world, N, V, c);
    for (int k = 0; k < 3; ++k) lit[k] = lit[k] + (base[k] * c[k] + c[3 + k]);
}
