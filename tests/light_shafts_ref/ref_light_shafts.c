/* ref_light_shafts.c (TEST INFRASTRUCTURE ONLY) -- C restatement of PassLightShafts::execute,
 * shs-renderer-lib/include/shs/passes/pass_light_shafts.hpp:44-215, the reference of tests/test_light_shafts.py.
 * Every step carries the line it restates.  std::max / std::clamp keep their comparison forms
 * ((a < b) ? b : a; (v < lo) ? lo : (hi < v) ? hi : v -- a NaN value passes through clamp), std::lround is
 * libm's lroundf (the pass's argument is a float), glm's mat4 * vec4 and vec3 / float keep glm's order of
 * operations.  Built with -ffp-contract=off: every float operation rounds once, as the reference build. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

static int max_i(int a, int b) { return (a < b) ? b : a; }                                   /* std::max */
static float max_f(float a, float b) { return (a < b) ? b : a; }
static int clamp_i(int v, int lo, int hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }      /* std::clamp */
static float clamp_f(float v, float lo, float hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }

/* :78-92.  sun_uv keeps its initial (0.5, 0.2) when |clip.w| <= 1e-6; returns sun_valid. */
int ref_sun_uv(const float cam_pos[3], const float sun_dir_ws[3], const float vp[16], float sun_uv[2]) {
    sun_uv[0] = 0.5f;                                                                         /* :78 */
    sun_uv[1] = 0.2f;
    int sun_valid = 0;                                                                        /* :79 */
    float p[3], clip[4];
    for (int k = 0; k < 3; ++k) p[k] = cam_pos[k] + (-sun_dir_ws[k]) * 100.0f;                /* :81 */
    /* :82  glm mat4 * vec4: (m[0] * x + m[1] * y) + (m[2] * z + m[3] * w), columns m[c], w = 1 */
    for (int r = 0; r < 4; ++r) clip[r] = (vp[r] * p[0] + vp[4 + r] * p[1]) + (vp[8 + r] * p[2] + vp[12 + r] * 1.0f);
    if (fabsf(clip[3]) > 1e-6f) {                                                             /* :83 */
        const float ndc[3] = {clip[0] / clip[3], clip[1] / clip[3], clip[2] / clip[3]};       /* :85 */
        sun_uv[0] = ndc[0] * 0.5f + 0.5f;                                                     /* :86 */
        sun_uv[1] = ndc[1] * 0.5f + 0.5f;
        sun_valid = (clip[3] > 0.0f) && (ndc[2] >= -1.0f && ndc[2] <= 1.0f) &&                /* :87-90 */
                    (sun_uv[0] >= 0.0f && sun_uv[0] <= 1.0f) && (sun_uv[1] >= 0.0f && sun_uv[1] <= 1.0f);
    }
    return sun_valid;
}

/* :108-215 for input == output and no rt_shafts_tmp (the adapter's case), the sun given on the screen.
 * ldr: w * h RGBA8, rows y up, rewritten in place; depth: w * h floats or NULL (no rt_depth_like);
 * boost_out: w * h ints or NULL (the per-pixel boost, for the tests' spread condition).
 * Returns 0, or -1 when the scratch planes cannot be allocated. */
int ref_light_shafts_uv(uint8_t *ldr, const float *depth, int w, int h, int steps_in, float density_in, float weight_in,
                        float decay_in, const float sun_uv[2], int32_t *boost_out) {
    const size_t n = (size_t)w * (size_t)h;
    float *luma = malloc(n * sizeof(float));                                                  /* :109-110 */
    uint8_t *scratch = malloc(n * 4);                                                         /* :138-139 */
    if (!luma || !scratch) {
        free(luma);
        free(scratch);
        return -1;
    }
    for (int y = 0; y < h; ++y) {                                                             /* :113-123 */
        for (int x = 0; x < w; ++x) {
            const uint8_t *c = ldr + ((size_t)y * w + x) * 4;                                 /* :117 */
            const float r = (float)c[0] / 255.0f;                                             /* :118 */
            const float g = (float)c[1] / 255.0f;                                             /* :119 */
            const float b = (float)c[2] / 255.0f;                                             /* :120 */
            luma[(size_t)y * w + x] = 0.2126f * r + 0.7152f * g + 0.0722f * b;                /* :121 */
        }
    }
    const int steps = max_i(8, steps_in);                                                     /* :133 */
    const float density = max_f(0.0f, density_in);                                            /* :134 */
    const float weight = max_f(0.0f, weight_in);                                              /* :135 */
    const float decay = clamp_f(decay_in, 0.0f, 1.0f);                                        /* :136 */
    for (int y = 0; y < h; ++y) {                                                             /* :143 */
        for (int x = 0; x < w; ++x) {                                                         /* :145 */
            const float u = (float)x / (float)max_i(1, w - 1);                                /* :147 */
            const float v = (float)y / (float)max_i(1, h - 1);                                /* :148 */
            float illum_decay = 1.0f;                                                         /* :150 */
            float accum = 0.0f;                                                               /* :151 */
            for (int i = 0; i < steps; ++i) {                                                 /* :152 */
                const float t = (float)i / (float)steps;                                      /* :154 */
                const float su = u + (sun_uv[0] - u) * t * density;                           /* :155 */
                const float sv = v + (sun_uv[1] - v) * t * density;                           /* :156 */
                const int sx = (int)lroundf(su * (float)(w - 1));                             /* :157 */
                const int sy = (int)lroundf(sv * (float)(h - 1));                             /* :158 */
                const int cx = clamp_i(sx, 0, w - 1), cy = clamp_i(sy, 0, h - 1);             /* :128-129, :164-165 */
                float s = luma[(size_t)cy * w + cx];                                          /* :160, :130 */
                if (depth) {                                                                  /* :161 */
                    const float d = depth[(size_t)cy * w + cx];                               /* :166 */
                    s *= clamp_f(d, 0.0f, 1.0f);                                              /* :167 */
                }
                accum += s * illum_decay * weight;                                            /* :170 */
                illum_decay *= decay;                                                         /* :171 */
            }
            const uint8_t *base = ldr + ((size_t)y * w + x) * 4;                              /* :174 */
            const int boost = clamp_i((int)lroundf(accum * 80.0f), 0, 120);                   /* :175 */
            uint8_t *out = scratch + ((size_t)y * w + x) * 4;                                 /* :183 */
            out[0] = (uint8_t)clamp_i((int)base[0] + boost, 0, 255);                          /* :177 */
            out[1] = (uint8_t)clamp_i((int)base[1] + boost, 0, 255);                          /* :178 */
            out[2] = (uint8_t)clamp_i((int)base[2] + boost / 2, 0, 255);                      /* :179 */
            out[3] = 255;                                                                     /* :180 */
            if (boost_out) boost_out[(size_t)y * w + x] = boost;
        }
    }
    for (size_t k = 0; k < n * 4; ++k) ldr[k] = scratch[k];                                   /* :202-213 */
    free(luma);
    free(scratch);
    return 0;
}

/* The whole pass as the "light_shafts" adapter runs it (:44-215, input == output): disabled (:54-56) or an
 * invalid sun (:95-97) leaves the LDR as it is.  Returns 1 when the shafts ran, 0 when the LDR was left,
 * -1 on allocation failure. */
int ref_light_shafts(uint8_t *ldr, const float *depth, int w, int h, int enable, int steps, float density, float weight,
                     float decay, const float cam_pos[3], const float sun_dir_ws[3], const float vp[16], int32_t *boost_out) {
    if (w <= 0 || h <= 0) return 0;                                                           /* :51 */
    if (!enable) return 0;                                                                    /* :54-56 */
    float sun_uv[2];
    if (!ref_sun_uv(cam_pos, sun_dir_ws, vp, sun_uv)) return 0;                               /* :78-97 */
    return ref_light_shafts_uv(ldr, depth, w, h, steps, density, weight, decay, sun_uv, boost_out) ? -1 : 1;
}
