// tests/canvas_light_shafts_ref (TEST INFRASTRUCTURE ONLY): a C restatement of light_shafts_pass of
// hello-render-target/hello_pbr_light_shafts.cpp (:1390-1707) with the helpers it calls -- shadow_uvz_from_world
// (:558-576), srgb_to_linear / linear_to_srgb / color_to_rgb01 / rgb01_to_color (hello-shs-renderer/shs_renderer.hpp
// :273-298) and Math::clamp / saturate (:130-145) -- one function per reference function, every float expression in
// the reference's order.  GLM's pieces are written out as GLM associates them: mat4 * vec4 sums its columns as
// (c0 x + c1 y) + (c2 z + c3 w), dot(vec3) is (x + y) + z, normalize multiplies by 1 / sqrt(dot), mix(x, y, a) is
// x * (1 - a) + y * a, clamp is min(max(x, lo), hi).  The reference of tests/test_canvas_light_shafts*.py.
//
// dbl: the six transcendentals (sin, cos, sin and exp per step, exp for Tm, pow(., 1.5) per pixel, pow(., 1 / 2.2) at
// the end) in double, rounded once to float, instead of the float libm's.
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "shs_gpu.h"

typedef struct { float x, y, z; } v3;
typedef shs_canvas_light_shafts_desc desc_t;

// per pixel, optional: what the pass derives before any transcendental
typedef struct rls_debug {
    float *ray_max;      // W*H (the copied pixels' too)
    float *view_dir;     // W*H*3 (marched pixels)
    float *steps;        // W*H*max(1, steps)*8: t, wp.xyz, uv.xy, z, vis of each visited step; the caller presets
                         // the plane, so what a step did not compute keeps the preset
    int32_t *visited;    // W*H: the steps the loop entered before its exit
} rls_debug;

static int g_dbl;
static float *g_step;    // the current step's debug record, or NULL

static float t_sin(float x) { return g_dbl ? (float)sin((double)x) : sinf(x); }
static float t_cos(float x) { return g_dbl ? (float)cos((double)x) : cosf(x); }
static float t_exp(float x) { return g_dbl ? (float)exp((double)x) : expf(x); }
static float t_pow(float x, float y) { return g_dbl ? (float)pow((double)x, (double)y) : powf(x, y); }

// srgb_to_linear of a byte's c / 255 (shs_renderer.hpp:273-276; the clamp changes nothing there): always the float
// libm's, which the pass under test reads from a table the host builds with the same call
static float t_lin(float srgb01) { return powf(srgb01, 2.2f); }

static float maxf(float a, float b) { return (a < b) ? b : a; }   // std::max, glm::max
static float minf(float a, float b) { return (b < a) ? b : a; }   // std::min, glm::min
static int maxi(int a, int b) { return (a < b) ? b : a; }
static int mini(int a, int b) { return (b < a) ? b : a; }
static float clampf(float v, float lo, float hi) { return (v < lo) ? lo : (v > hi ? hi : v); }   // Math::clamp
static float gclamp(float x, float lo, float hi) { return minf(maxf(x, lo), hi); }               // glm::clamp

static void mat4_mul_vec4(const float *m, float x, float y, float z, float w, float *o) {
    for (int r = 0; r < 4; ++r) o[r] = (m[r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r] * w);
}
static float dot3(v3 a, v3 b) { float x = a.x * b.x, y = a.y * b.y, z = a.z * b.z; return (x + y) + z; }

// :1395-1420
static v3 reconstruct_world_dir_from_pixel(int x, int y, int W, int H, const float *inv_vp, v3 cam_pos) {
    const v3 fwd = {0.0f, 0.0f, 1.0f};
    int py_screen = (H - 1) - y;
    float fx = ((float)x + 0.5f) / (float)W;
    float fy = ((float)py_screen + 0.5f) / (float)H;
    float ndc_x = fx * 2.0f - 1.0f;
    float ndc_y = 1.0f - fy * 2.0f;
    float wf[4];
    mat4_mul_vec4(inv_vp, ndc_x, ndc_y, 1.0f, 1.0f, wf);
    if (fabsf(wf[3]) < 1e-8f) return fwd;
    wf[0] /= wf[3];
    wf[1] /= wf[3];
    wf[2] /= wf[3];
    v3 dir = {wf[0] - cam_pos.x, wf[1] - cam_pos.y, wf[2] - cam_pos.z};
    float len = sqrtf(dot3(dir, dir));
    if (len < 1e-6f) return fwd;
    v3 out = {dir.x / len, dir.y / len, dir.z / len};
    return out;
}

// :1423-1429
static float fog_density(const desc_t *p, v3 world_pos) {
    float y = world_pos.y;
    float h = maxf(0.0f, y);
    float d = p->base_density * t_exp(-h * p->height_falloff);
    return d;
}

// :1432-1440
static float phase_hg(float cosTheta, float g) {
    cosTheta = clampf(cosTheta, -1.0f, 1.0f);
    g = clampf(g, -0.95f, 0.95f);
    float gg = g * g;
    float denom = t_pow(maxf(1e-4f, 1.0f + gg - 2.0f * g * cosTheta), 1.5f);
    return (1.0f - gg) / denom;
}

// :1443-1448
static float shadow_sample_depth_raw(const float *shadow_raw, int sw, int sh, int x, int y) {
    x = maxi(0, mini(sw - 1, x));
    y = maxi(0, mini(sh - 1, y));
    return shadow_raw[(size_t)y * (size_t)sw + (size_t)x];
}

// :1450-1464
static float shadow_compare_raw(const float *shadow_raw, int sw, int sh, float u, float v, float z_ndc, float bias) {
    if (!shadow_raw || sw <= 0 || sh <= 0) return 1.0f;
    if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) return 1.0f;
    int x = (int)lroundf(u * (float)(sw - 1));
    int y = (int)lroundf(v * (float)(sh - 1));
    float d = shadow_sample_depth_raw(shadow_raw, sw, sh, x, y);
    if (d == FLT_MAX) return 1.0f;
    return (z_ndc <= d + bias) ? 1.0f : 0.0f;
}

static float cmp_depth(float d, float z_ndc, float bias) {
    if (d == FLT_MAX) return 1.0f;
    return (z_ndc <= d + bias) ? 1.0f : 0.0f;
}

// :1466-1492
static float shadow_factor_pcf_2x2_raw(const float *shadow_raw, int sw, int sh, float u, float v, float z_ndc, float bias,
                                       int enable_pcf) {
    if (!enable_pcf) return shadow_compare_raw(shadow_raw, sw, sh, u, v, z_ndc, bias);
    if (!shadow_raw || sw <= 0 || sh <= 0) return 1.0f;
    float fx = u * (float)(sw - 1);
    float fy = v * (float)(sh - 1);
    int x0 = maxi(0, mini(sw - 1, (int)floorf(fx)));
    int y0 = maxi(0, mini(sh - 1, (int)floorf(fy)));
    int x1 = maxi(0, mini(sw - 1, x0 + 1));
    int y1 = maxi(0, mini(sh - 1, y0 + 1));
    float d00 = shadow_sample_depth_raw(shadow_raw, sw, sh, x0, y0);
    float d10 = shadow_sample_depth_raw(shadow_raw, sw, sh, x1, y0);
    float d01 = shadow_sample_depth_raw(shadow_raw, sw, sh, x0, y1);
    float d11 = shadow_sample_depth_raw(shadow_raw, sw, sh, x1, y1);
    return 0.25f * (cmp_depth(d00, z_ndc, bias) + cmp_depth(d10, z_ndc, bias) + cmp_depth(d01, z_ndc, bias) +
                    cmp_depth(d11, z_ndc, bias));
}

// :558-576
static int shadow_uvz_from_world(const float *light_vp, v3 world_pos, float *out_u, float *out_v, float *out_z_ndc) {
    float clip[4];
    mat4_mul_vec4(light_vp, world_pos.x, world_pos.y, world_pos.z, 1.0f, clip);
    if (fabsf(clip[3]) < 1e-6f) return 0;
    float nx = clip[0] / clip[3], ny = clip[1] / clip[3], nz = clip[2] / clip[3];
    *out_z_ndc = nz;
    if (g_step) g_step[6] = nz;
    if (*out_z_ndc < 0.0f || *out_z_ndc > 1.0f) return 0;
    *out_u = nx * 0.5f + 0.5f;
    *out_v = 1.0f - (ny * 0.5f + 0.5f);
    if (g_step) {
        g_step[4] = *out_u;
        g_step[5] = *out_v;
    }
    return 1;
}

// :1494-1507
static float volumetric_shadow_visibility(const desc_t *p, const float *shadow_raw, int sw, int sh, const float *light_vp,
                                          v3 world_pos) {
    if (!p->use_shadow || !shadow_raw) return 1.0f;
    float u, v, z;
    if (!shadow_uvz_from_world(light_vp, world_pos, &u, &v, &z)) return 1.0f;
    return shadow_factor_pcf_2x2_raw(shadow_raw, sw, sh, u, v, z, p->shadow_bias, p->shadow_pcf_2x2);
}

// :1516-1522
static float volumetric_cloud_noise(v3 p, float scale) {
    v3 s = {p.x * scale, p.y * scale, p.z * scale};
    float n = t_sin(s.x) * t_cos(s.y) * t_sin(s.z + s.x * 0.5f);
    return n * 0.5f + 0.5f;
}

// light_shafts_pass (:1525-1707), the tiles' pixels in any order (a pixel reads only its own).  src / dst: W*H Color,
// depth W*H view z, shadow_raw shadow_w * shadow_h or NULL.  pq (may be NULL): W*H*4 -- outSrgb * 255 before the
// byte truncation and the number of steps that entered the second `dens > 1e-6f` block, (0, 0, 0, -1) for a pixel
// the pass only copies.
int rls_pass(const desc_t *p, const uint8_t *src, const float *depth, const float *shadow_raw, uint8_t *dst, float *pq, int dbl,
             const rls_debug *dbg) {
    const v3 shafts_tint = {0.92f, 0.96f, 1.00f};
    const v3 ambient_tint = {0.60f, 0.65f, 0.70f};
    const int W = p->width, H = p->height;
    const v3 cam_pos = {p->cam_pos[0], p->cam_pos[1], p->cam_pos[2]};
    g_dbl = dbl;
    v3 sun_dir;
    {   // -glm::normalize(sun_dir_world)
        const v3 s = {p->sun_dir_world[0], p->sun_dir_world[1], p->sun_dir_world[2]};
        const float inv = 1.0f / sqrtf(dot3(s, s));
        sun_dir.x = -(s.x * inv);
        sun_dir.y = -(s.y * inv);
        sun_dir.z = -(s.z * inv);
    }
    const int nsteps = maxi(1, p->steps);
    for (int y = 0; y < H; ++y) {
        int row = y * W;
        for (int x = 0; x < W; ++x) {
            const uint8_t *base_srgb = src + 4 * (size_t)(row + x);
            uint8_t *out = dst + 4 * (size_t)(row + x);
            float *opq = pq ? pq + 4 * (size_t)(row + x) : NULL;
            uint8_t base[4] = {base_srgb[0], base_srgb[1], base_srgb[2], base_srgb[3]};
            if (!p->enable) {
                for (int c = 0; c < 4; ++c) out[c] = base[c];
                if (opq) opq[0] = opq[1] = opq[2] = 0.0f, opq[3] = -1.0f;
                continue;
            }
            float view_z = depth[row + x];
            float ray_max = p->max_dist;
            if (view_z != FLT_MAX) ray_max = minf(ray_max, maxf(p->min_dist, view_z - 0.25f));
            if (dbg && dbg->ray_max) dbg->ray_max[row + x] = ray_max;
            if (ray_max <= p->min_dist) {
                for (int c = 0; c < 4; ++c) out[c] = base[c];
                if (opq) opq[0] = opq[1] = opq[2] = 0.0f, opq[3] = -1.0f;
                continue;
            }
            v3 view_dir = reconstruct_world_dir_from_pixel(x, y, W, H, p->inv_view_proj, cam_pos);
            if (dbg && dbg->view_dir) {
                dbg->view_dir[3 * (size_t)(row + x) + 0] = view_dir.x;
                dbg->view_dir[3 * (size_t)(row + x) + 1] = view_dir.y;
                dbg->view_dir[3 * (size_t)(row + x) + 2] = view_dir.z;
            }
            float cosTheta = dot3(view_dir, sun_dir);
            float phase = phase_hg(cosTheta, p->g);
            float gate = clampf((cosTheta - 0.1f) / 0.9f, 0.0f, 1.0f);
            int steps = nsteps;
            float ds = ray_max / (float)steps;
            uint32_t seed = (uint32_t)(x * 1973u ^ y * 9277u);
            float random_val = (float)(seed & 0xFFFF) / 65536.0f;
            float t = p->min_dist + (random_val * ds * p->jitter_amount);
            float Tm = 1.0f;
            v3 Ls = {0.0f, 0.0f, 0.0f};
            int accumulated = 0, visited = 0;
            for (int i = 0; i < steps; ++i) {
                if (t >= ray_max) break;
                v3 wp = {cam_pos.x + view_dir.x * t, cam_pos.y + view_dir.y * t, cam_pos.z + view_dir.z * t};
                g_step = (dbg && dbg->steps) ? dbg->steps + 8 * ((size_t)(row + x) * nsteps + i) : NULL;
                if (g_step) g_step[0] = t, g_step[1] = wp.x, g_step[2] = wp.y, g_step[3] = wp.z;
                ++visited;
                float dens = fog_density(p, wp);
                if (dens > 1e-6f) {
                    float dust = volumetric_cloud_noise(wp, p->noise_scale);
                    dens *= 1.0f * (1.0f - p->noise_strength) + dust * p->noise_strength;
                }
                if (dens > 1e-6f) {
                    float vis = volumetric_shadow_visibility(p, shadow_raw, p->shadow_w, p->shadow_h, p->light_vp, wp);
                    if (g_step) g_step[7] = vis;
                    float sigma_s = p->sigma_s * dens;
                    float sigma_t = p->sigma_t * dens;
                    float direct_light = phase * vis * gate;
                    float ambient_light = p->ambient_strength;
                    float light_term = (direct_light * p->intensity) + ambient_light;
                    float scatter = Tm * sigma_s * light_term * ds;
                    float dist01 = t / maxf(1e-3f, p->max_dist);
                    float dist_fall = 1.0f - (dist01 * dist01);
                    scatter *= dist_fall;
                    v3 tint = {ambient_tint.x * (1.0f - vis) + shafts_tint.x * vis, ambient_tint.y * (1.0f - vis) + shafts_tint.y * vis,
                               ambient_tint.z * (1.0f - vis) + shafts_tint.z * vis};
                    Ls.x += tint.x * scatter;
                    Ls.y += tint.y * scatter;
                    Ls.z += tint.z * scatter;
                    Tm *= t_exp(-sigma_t * ds);
                    ++accumulated;
                    if (Tm < 0.01f) break;
                }
                t += ds;
            }
            g_step = NULL;
            if (dbg && dbg->visited) dbg->visited[row + x] = visited;
            const float ls[3] = {Ls.x, Ls.y, Ls.z};
            for (int c = 0; c < 3; ++c) {
                float base01 = (float)base[c] / 255.0f;                            // color_to_rgb01
                float baseLin = t_lin(base01);
                float outLin = baseLin + ls[c];
                outLin = outLin / (1.0f + outLin * 0.15f);
                outLin = gclamp(outLin, 0.0f, 1.0f);
                float outSrgb = t_pow(gclamp(outLin, 0.0f, 1.0f), 1.0f / 2.2f);    // linear_to_srgb
                float c255 = gclamp(outSrgb, 0.0f, 1.0f) * 255.0f;                 // rgb01_to_color
                out[c] = (uint8_t)c255;
                if (opq) opq[c] = c255;
            }
            out[3] = 255;
            if (opq) opq[3] = (float)accumulated;
        }
    }
    return 0;
}

size_t rls_sizeof_desc(void) { return sizeof(desc_t); }
