/* tests/sky_ref (TEST INFRASTRUCTURE ONLY): a C restatement of the reference's sky models and of the pass
 * that paints them, the reference of tests/test_sky.py.  Cited lines are under
 * shs-renderer-lib/include/shs/: sky/procedural_sky.hpp, sky/cubemap_sky.hpp, sky/skybox_renderer.hpp.
 * GLM's operation orders (glm/detail/func_geometric.inl, func_common.inl, func_matrix.inl,
 * type_mat4x4.inl): dot(vec3) = (x + y) + z of the products, normalize = v * (1 / sqrt(dot)),
 * length = sqrt(dot), mix = x * (1 - a) + y * a, min(x, y) = y < x ? y : x, max(x, y) = x < y ? y : x,
 * clamp = min(max(x, lo), hi), mat4 * vec4 = (m0 x + m1 y) + (m2 z + m3 w).
 * Built without contraction or fast math: every float operation rounds once. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

typedef struct ref_sky {
    int32_t model;              /* 1 ProceduralSky, 2 CubemapSky */
    float sun_dir_ws[3];        /* ProceduralSky's constructor argument */
    float intensity;            /* CubemapSky */
    int32_t fw[6], fh[6];       /* faces +X,-X,+Y,-Y,+Z,-Z: RGBA8 texels, (x, y) at 4 * (y * w + x) */
    const uint8_t *face[6];     /* NULL: a Texture2DData that fails valid() */
} ref_sky;

typedef struct { float x, y, z; } v3;

static float g_min(float x, float y) { return (y < x) ? y : x; }
static float g_max(float x, float y) { return (x < y) ? y : x; }
static float g_clamp(float x, float lo, float hi) { return g_min(g_max(x, lo), hi); }
static float g_mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }
static v3 mix3(v3 a, v3 b, float t) { v3 r = {g_mix(a.x, b.x, t), g_mix(a.y, b.y, t), g_mix(a.z, b.z, t)}; return r; }
static float dot3(v3 a, v3 b) { const float x = a.x * b.x, y = a.y * b.y, z = a.z * b.z; return (x + y) + z; }
static v3 normalize3(v3 v) { const float inv = 1.0f / sqrtf(dot3(v, v)); v3 r = {v.x * inv, v.y * inv, v.z * inv}; return r; }

/* glm::inverse(mat4) (func_matrix.inl compute_inverse<4, 4>); column-major m[c * 4 + r] */
void ref_inverse(const float *mm, float *out) {
#define M(c, r) mm[(c) * 4 + (r)]
    const float c00 = M(2, 2) * M(3, 3) - M(3, 2) * M(2, 3);
    const float c02 = M(1, 2) * M(3, 3) - M(3, 2) * M(1, 3);
    const float c03 = M(1, 2) * M(2, 3) - M(2, 2) * M(1, 3);
    const float c04 = M(2, 1) * M(3, 3) - M(3, 1) * M(2, 3);
    const float c06 = M(1, 1) * M(3, 3) - M(3, 1) * M(1, 3);
    const float c07 = M(1, 1) * M(2, 3) - M(2, 1) * M(1, 3);
    const float c08 = M(2, 1) * M(3, 2) - M(3, 1) * M(2, 2);
    const float c10 = M(1, 1) * M(3, 2) - M(3, 1) * M(1, 2);
    const float c11 = M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2);
    const float c12 = M(2, 0) * M(3, 3) - M(3, 0) * M(2, 3);
    const float c14 = M(1, 0) * M(3, 3) - M(3, 0) * M(1, 3);
    const float c15 = M(1, 0) * M(2, 3) - M(2, 0) * M(1, 3);
    const float c16 = M(2, 0) * M(3, 2) - M(3, 0) * M(2, 2);
    const float c18 = M(1, 0) * M(3, 2) - M(3, 0) * M(1, 2);
    const float c19 = M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2);
    const float c20 = M(2, 0) * M(3, 1) - M(3, 0) * M(2, 1);
    const float c22 = M(1, 0) * M(3, 1) - M(3, 0) * M(1, 1);
    const float c23 = M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1);
    const float f0[4] = {c00, c00, c02, c03}, f1[4] = {c04, c04, c06, c07}, f2[4] = {c08, c08, c10, c11};
    const float f3[4] = {c12, c12, c14, c15}, f4[4] = {c16, c16, c18, c19}, f5[4] = {c20, c20, c22, c23};
    const float v0[4] = {M(1, 0), M(0, 0), M(0, 0), M(0, 0)};
    const float v1[4] = {M(1, 1), M(0, 1), M(0, 1), M(0, 1)};
    const float v2[4] = {M(1, 2), M(0, 2), M(0, 2), M(0, 2)};
    const float v3_[4] = {M(1, 3), M(0, 3), M(0, 3), M(0, 3)};
    const float sa[4] = {+1.f, -1.f, +1.f, -1.f}, sb[4] = {-1.f, +1.f, -1.f, +1.f};
    float inv[4][4];
    for (int i = 0; i < 4; ++i) {
        inv[0][i] = ((v1[i] * f0[i] - v2[i] * f1[i]) + v3_[i] * f2[i]) * sa[i];
        inv[1][i] = ((v0[i] * f0[i] - v2[i] * f3[i]) + v3_[i] * f4[i]) * sb[i];
        inv[2][i] = ((v0[i] * f1[i] - v1[i] * f3[i]) + v3_[i] * f5[i]) * sa[i];
        inv[3][i] = ((v0[i] * f2[i] - v1[i] * f4[i]) + v2[i] * f5[i]) * sb[i];
    }
    const float d0 = M(0, 0) * inv[0][0], d1 = M(0, 1) * inv[1][0], d2 = M(0, 2) * inv[2][0], d3 = M(0, 3) * inv[3][0];
    const float det = (d0 + d1) + (d2 + d3);
    const float one_over = 1.0f / det;
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) out[c * 4 + r] = inv[c][r] * one_over;
#undef M
}

/* procedural_sky.hpp:26-46; sun = the constructor's normalize(sun_dir_ws) (:23) */
static v3 procedural_sample(v3 sun, v3 direction_ws) {
    const v3 d = normalize3(direction_ws);                                  /* :28 */
    const float t = g_clamp(d.y * 0.5f + 0.5f, 0.0f, 1.0f);                 /* :29 */
    const v3 zenith = {0.05f, 0.20f, 0.50f};                                /* :31 */
    const v3 horizon = {0.30f, 0.60f, 1.00f};                               /* :32 */
    v3 sky = mix3(horizon, zenith, t);                                      /* :33 */
    const v3 nsun = {-sun.x, -sun.y, -sun.z};
    const float sun_dot = dot3(d, nsun);                                    /* :35 */
    if (sun_dot > 0.9998f) {                                                /* :36 */
        const v3 disc = {15.0f, 15.0f, 15.0f};
        sky = disc;                                                         /* :38 */
    } else if (sun_dot > 0.9990f) {                                         /* :40 */
        const float glow = (sun_dot - 0.9990f) / (0.9998f - 0.9990f);       /* :42 */
        const v3 ring = {10.0f, 8.0f, 4.0f};
        sky = mix3(sky, ring, glow);                                        /* :43 */
    }
    return sky;
}

/* cubemap_sky.hpp:39-45 */
static v3 srgb_to_linear_approx(const uint8_t *c) {
    const float gamma = 2.2f;
    v3 r = {powf((float)c[0] / 255.0f, gamma), powf((float)c[1] / 255.0f, gamma), powf((float)c[2] / 255.0f, gamma)};
    return r;
}

/* cubemap_sky.hpp:47-71 */
static v3 sample_face_bilinear_linear(const uint8_t *tex, int w, int h, float u, float v) {
    const v3 zero = {0.0f, 0.0f, 0.0f};
    if (!tex || w <= 0 || h <= 0) return zero;                              /* :49 */
    u = g_clamp(u, 0.0f, 1.0f);                                             /* :51 */
    v = g_clamp(v, 0.0f, 1.0f);
    const float fx = u * (float)(w - 1);                                    /* :54 */
    const float fy = v * (float)(h - 1);
    const int x0 = (int)floorf(fx);                                         /* :56 */
    const int y0 = (int)floorf(fy);
    const int x1 = (x0 + 1 < w - 1) ? x0 + 1 : w - 1;                       /* :58 std::min */
    const int y1 = (y0 + 1 < h - 1) ? y0 + 1 : h - 1;
    const float tx = fx - (float)x0;                                        /* :60 */
    const float ty = fy - (float)y0;
#define AT(x, y) (tex + 4 * ((size_t)(y) * (size_t)w + (size_t)(x)))
    const v3 v00 = srgb_to_linear_approx(AT(x0, y0));                       /* :63-66 */
    const v3 v10 = srgb_to_linear_approx(AT(x1, y0));
    const v3 v01 = srgb_to_linear_approx(AT(x0, y1));
    const v3 v11 = srgb_to_linear_approx(AT(x1, y1));
#undef AT
    const v3 vx0 = mix3(v00, v10, tx);                                      /* :68 */
    const v3 vx1 = mix3(v01, v11, tx);
    return mix3(vx0, vx1, ty);                                              /* :70 */
}

/* cubemap_sky.hpp:80-116 */
static v3 cubemap_sample(const ref_sky *s, v3 direction_ws) {
    const v3 zero = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 6; ++i)
        if (!s->face[i] || s->fw[i] <= 0 || s->fh[i] <= 0) return zero;     /* :82 CubemapData::valid (:29-36) */
    v3 d = direction_ws;
    const float len = sqrtf(dot3(d, d));                                    /* :85 */
    if (len < 1e-8f) return zero;                                           /* :86 */
    d.x /= len; d.y /= len; d.z /= len;                                     /* :87 */
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);          /* :89-91 */
    int face = 0;
    float u = 0.5f, v = 0.5f;
    if (ax >= ay && ax >= az) {                                             /* :97 */
        if (d.x > 0.0f) { face = 0; u = (-d.z / ax); v = (d.y / ax); }
        else            { face = 1; u = (d.z / ax); v = (d.y / ax); }
    } else if (ay >= ax && ay >= az) {                                      /* :102 */
        if (d.y > 0.0f) { face = 2; u = (d.x / ay); v = (-d.z / ay); }
        else            { face = 3; u = (d.x / ay); v = (d.z / ay); }
    } else {
        if (d.z > 0.0f) { face = 4; u = (d.x / az); v = (d.y / az); }
        else            { face = 5; u = (-d.x / az); v = (d.y / az); }
    }
    u = 0.5f * (u + 1.0f);                                                  /* :113 */
    v = 0.5f * (v + 1.0f);
    const v3 c = sample_face_bilinear_linear(s->face[face], s->fw[face], s->fh[face], u, v);
    const v3 r = {c.x * s->intensity, c.y * s->intensity, c.z * s->intensity};   /* :115 */
    return r;
}

static v3 sky_sample(const ref_sky *s, v3 sun, v3 d) { return s->model == 1 ? procedural_sample(sun, d) : cubemap_sample(s, d); }

static v3 sun_of(const ref_sky *s) {
    const v3 raw = {s->sun_dir_ws[0], s->sun_dir_ws[1], s->sun_dir_ws[2]};
    return normalize3(raw);                                                 /* procedural_sky.hpp:23 */
}

/* ISkyModel::sample for n directions (dirs, rgb: n x 3 floats) */
void ref_sky_sample(const ref_sky *s, const float *dirs, int n, float *rgb) {
    const v3 sun = sun_of(s);
    for (int i = 0; i < n; ++i) {
        const v3 d = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
        const v3 c = sky_sample(s, sun, d);
        rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
    }
}

/* render_skybox_to_hdr (skybox_renderer.hpp:25-57) into hdr[(y * w + x) * 4], the RT_ColorHDR's own rows */
void ref_sky_fill(const ref_sky *s, const float *viewproj, const float *cam_pos, int w, int h, float *hdr) {
    if (w <= 0 || h <= 0) return;                                           /* :27 */
    float inv_vp[16];
    ref_inverse(viewproj, inv_vp);                                          /* :29 */
    const v3 cam = {cam_pos[0], cam_pos[1], cam_pos[2]};
    const v3 sun = sun_of(s);
    for (int y = 0; y < h; ++y) {
        const float ndc_y = (2.0f * ((float)y + 0.5f) / (float)h) - 1.0f;   /* :38 */
        for (int x = 0; x < w; ++x) {
            const float ndc_x = (2.0f * ((float)x + 0.5f) / (float)w) - 1.0f;   /* :41 */
            float *o = hdr + ((size_t)y * (size_t)w + (size_t)x) * 4;
            const float cx = ndc_x, cy = ndc_y, cz = 1.0f, cw = 1.0f;       /* :42 */
            float world[4];
            for (int r = 0; r < 4; ++r)                                     /* :43 */
                world[r] = (inv_vp[r] * cx + inv_vp[4 + r] * cy) + (inv_vp[8 + r] * cz + inv_vp[12 + r] * cw);
            if (fabsf(world[3]) < 1e-8f) {                                  /* :44 */
                o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; o[3] = 1.0f;
                continue;
            }
            const float ww = world[3];
            world[0] /= ww; world[1] /= ww; world[2] /= ww; world[3] /= ww; /* :49 */
            const v3 rel = {world[0] - cam.x, world[1] - cam.y, world[2] - cam.z};
            const v3 c = sky_sample(s, sun, normalize3(rel));               /* :51-52 */
            o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = 1.0f;                /* :53 */
        }
    }
}
