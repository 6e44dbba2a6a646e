/* tests/canvas_fx_ref (TEST INFRASTRUCTURE ONLY): a C restatement of the Canvas-API post passes of three
 * render-target demos, written from the cited lines (paths relative to cpp-folders/src/hello-render-target/):
 *   rfx_velocity_blur  motion_blur_pass            hello_multi_pass.cpp:605-683 (= hello_glowing_star.cpp:441-523)
 *   rfx_fog            fog_pass                    hello_multi_pass.cpp:764-819, smoothstep01 / lerp_color :120-137
 *   rfx_outline        outline_pass                hello_multi_pass.cpp:689-758
 *   rfx_fxaa           fxaa_pass                   hello_multi_pass.cpp:1000-1114, luma_from_color :159-165
 *   rfx_spec_bright    build_spec_bright_pass      hello_glowing_star.cpp:700-752
 *   rfx_additive       additive_composite_pass     hello_glowing_star.cpp:754-795, mul_color / add_color_clamped :146-164
 *   rfx_lens_flare     pseudo_lens_flare_pass      hello_glowing_star.cpp:802-906
 * The tile jobs of the reference write disjoint pixels from a read-only source, so a plain loop over the pixels
 * gives their result.  Canvases are W*H RGBA bytes at y * W + x; float -> integer conversions are the x86-64
 * build's (cvttss2si: NaN and out-of-range give INT_MIN; a float -> uint8_t keeps the low byte of that).
 * The fog's pow and the flare's exp are the host's float libm, as the reference's; with dbl != 0 they are the
 * function in double rounded once to float, which is what the GPU kernels evaluate.
 * branch (may be NULL): one byte per pixel saying which way the pass went (the RFX_* values below). */
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "shs_gpu.h"

enum { RFX_FOG_COPIED = 0, RFX_FOG_T0 = 1, RFX_FOG_INTERIOR = 2, RFX_FOG_T1 = 3 };
enum { RFX_OUTLINE_COPIED = 0, RFX_OUTLINE_EDGE = 1, RFX_OUTLINE_FLAT = 2 };
enum { RFX_FXAA_LOW_CONTRAST = 0, RFX_FXAA_RGBA = 1, RFX_FXAA_RGBB = 2 };
enum { RFX_FLARE_OFF_CENTRE = 0, RFX_FLARE_CENTRE = 1 };

typedef struct { uint8_t r, g, b, a; } Color;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
static float min_f(float a, float b) { return (b < a) ? b : a; }   /* std::min */
static float max_f(float a, float b) { return (a < b) ? b : a; }   /* std::max */
static int int_x86(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN; }
static uint8_t u8_x86(float f) { return (uint8_t)int_x86(f); }
static int round_i(float v) { return int_x86(roundf(v)); }

static float smoothstep01(float t) {
    t = clampf(t, 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}

static Color color_from_rgbaf(float r, float g, float b, float a) {
    r = min_f(255.0f, max_f(0.0f, r));
    g = min_f(255.0f, max_f(0.0f, g));
    b = min_f(255.0f, max_f(0.0f, b));
    a = min_f(255.0f, max_f(0.0f, a));
    return (Color){u8_x86(r), u8_x86(g), u8_x86(b), u8_x86(a)};
}

static float luma_from_color(Color c) {
    const float r = (float)c.r / 255.0f, g = (float)c.g / 255.0f, b = (float)c.b / 255.0f;
    return 0.299f * r + 0.587f * g + 0.114f * b;
}

static Color get(const Color *c, int W, int H, int x, int y) {
    (void)H;
    return c[(size_t)y * W + x];
}

static Color sample_i(const Color *c, int W, int H, int sx, int sy) {
    return get(c, W, H, clampi(sx, 0, W - 1), clampi(sy, 0, H - 1));
}

static Color sample_f(const Color *c, int W, int H, float fx, float fy) {
    return get(c, W, H, clampi(round_i(fx), 0, W - 1), clampi(round_i(fy), 0, H - 1));
}

size_t rfx_sizeof_descs(int which) {
    switch (which) {
    case 0: return sizeof(shs_canvas_velocity_blur_desc);
    case 1: return sizeof(shs_canvas_fog_desc);
    case 2: return sizeof(shs_canvas_outline_desc);
    case 3: return sizeof(shs_canvas_fxaa_desc);
    case 4: return sizeof(shs_canvas_spec_bright_desc);
    case 5: return sizeof(shs_canvas_lens_flare_desc);
    case 6: return sizeof(shs_canvas_multi_pass_frame_desc);
    case 7: return sizeof(shs_canvas_glow_frame_desc);
    default: return 0;
    }
}

void rfx_velocity_blur(const shs_canvas_velocity_blur_desc *d, const uint8_t *src8, const float *velocity, uint8_t *dst8) {
    const int W = d->width, H = d->height, samples = d->samples;
    const Color *src = (const Color *)src8;
    Color *dst = (Color *)dst8;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const float vx = velocity[2 * i] * d->strength, vy = velocity[2 * i + 1] * d->strength;
            const float vlen = sqrtf(vx * vx + vy * vy);
            if (vlen < 0.001f || samples <= 1) {
                dst[i] = src[i];
                continue;
            }
            const float dirx = vx / vlen, diry = vy / vlen;
            float r = 0, g = 0, b = 0, wsum = 0.0f;
            for (int k = 0; k < samples; ++k) {
                const float t = (samples == 1) ? 0.0f : ((float)k / (float)(samples - 1));
                const float a = (t - 0.5f) * 2.0f;
                const float px = (float)x + dirx * (a * vlen), py = (float)y + diry * (a * vlen);
                const Color c = sample_f(src, W, H, px, py);
                const float wgt = 1.0f - fabsf(a);
                r += wgt * (float)c.r;
                g += wgt * (float)c.g;
                b += wgt * (float)c.b;
                wsum += wgt;
            }
            if (wsum < 0.0001f) wsum = 1.0f;
            dst[i] = (Color){(uint8_t)clampi(int_x86(r / wsum), 0, 255), (uint8_t)clampi(int_x86(g / wsum), 0, 255),
                             (uint8_t)clampi(int_x86(b / wsum), 0, 255), 255};
        }
}

void rfx_fog(const shs_canvas_fog_desc *d, const uint8_t *src8, const float *depth, uint8_t *dst8, float *pq, int dbl,
             uint8_t *branch) {
    const int W = d->width, H = d->height;
    const Color *src = (const Color *)src8;
    Color *dst = (Color *)dst8;
    const Color fog = {d->fog_color[0], d->fog_color[1], d->fog_color[2], d->fog_color[3]};
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const Color c = src[i];
        const float z = depth[i];
        if (z == FLT_MAX) {
            dst[i] = c;
            if (pq) pq[4 * i] = pq[4 * i + 1] = pq[4 * i + 2] = 0.0f, pq[4 * i + 3] = -1.0f;
            if (branch) branch[i] = RFX_FOG_COPIED;
            continue;
        }
        float t = (z - d->fog_start) / (d->fog_end - d->fog_start);
        t = smoothstep01(t);
        t = dbl ? (float)pow((double)t, (double)d->fog_power) : powf(t, d->fog_power);
        /* lerp_color */
        t = clampf(t, 0.0f, 1.0f);
        const float ia = 1.0f - t;
        const float r = ia * c.r + t * fog.r, g = ia * c.g + t * fog.g, b = ia * c.b + t * fog.b;
        dst[i] = (Color){u8_x86(r), u8_x86(g), u8_x86(b), 255};
        if (pq) pq[4 * i] = r, pq[4 * i + 1] = g, pq[4 * i + 2] = b, pq[4 * i + 3] = 1.0f;
        if (branch) branch[i] = (t == 0.0f) ? RFX_FOG_T0 : (t == 1.0f ? RFX_FOG_T1 : RFX_FOG_INTERIOR);
    }
}

void rfx_outline(const shs_canvas_outline_desc *d, const uint8_t *src8, const float *depth, uint8_t *dst8, uint8_t *branch) {
    const int W = d->width, H = d->height, R = d->radius;
    const Color *src = (const Color *)src8;
    Color *dst = (Color *)dst8;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const Color c = src[i];
            const float d0 = depth[i];
            if (d0 == FLT_MAX) {
                dst[i] = c;
                if (branch) branch[i] = RFX_OUTLINE_COPIED;
                continue;
            }
            float max_delta = 0.0f;
            for (int oy = -R; oy <= R; ++oy)
                for (int ox = -R; ox <= R; ++ox) {
                    if (ox == 0 && oy == 0) continue;
                    const int sx = clampi(x + ox, 0, W - 1), sy = clampi(y + oy, 0, H - 1);
                    const float d1 = depth[(size_t)sy * W + sx];
                    if (d1 == FLT_MAX) continue;
                    max_delta = max_f(max_delta, fabsf(d1 - d0));
                }
            const float edge = (max_delta > d->threshold) ? 1.0f : 0.0f;
            const float k = 1.0f - edge * d->strength;
            dst[i] = (Color){(uint8_t)clampi(int_x86((float)c.r * k), 0, 255), (uint8_t)clampi(int_x86((float)c.g * k), 0, 255),
                             (uint8_t)clampi(int_x86((float)c.b * k), 0, 255), 255};
            if (branch) branch[i] = (edge != 0.0f) ? RFX_OUTLINE_EDGE : RFX_OUTLINE_FLAT;
        }
}

void rfx_fxaa(const shs_canvas_fxaa_desc *d, const uint8_t *src8, uint8_t *dst8, uint8_t *branch) {
    const int W = d->width, H = d->height;
    const Color *src = (const Color *)src8;
    Color *dst = (Color *)dst8;
    const float REDUCE_MIN = d->reduce_min, REDUCE_MUL = d->reduce_mul, SPAN_MAX = d->span_max;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const Color rgbM = sample_i(src, W, H, x, y);
            const Color rgbNW = sample_i(src, W, H, x - 1, y + 1), rgbNE = sample_i(src, W, H, x + 1, y + 1);
            const Color rgbSW = sample_i(src, W, H, x - 1, y - 1), rgbSE = sample_i(src, W, H, x + 1, y - 1);
            const float lumaM = luma_from_color(rgbM);
            const float lumaNW = luma_from_color(rgbNW), lumaNE = luma_from_color(rgbNE);
            const float lumaSW = luma_from_color(rgbSW), lumaSE = luma_from_color(rgbSE);
            const float lumaMin = min_f(lumaM, min_f(min_f(lumaNW, lumaNE), min_f(lumaSW, lumaSE)));
            const float lumaMax = max_f(lumaM, max_f(max_f(lumaNW, lumaNE), max_f(lumaSW, lumaSE)));
            const float contrast = lumaMax - lumaMin;
            if (contrast < 0.02f) {
                dst[i] = rgbM;
                if (branch) branch[i] = RFX_FXAA_LOW_CONTRAST;
                continue;
            }
            float dirx = -((lumaNW + lumaNE) - (lumaSW + lumaSE));
            float diry = ((lumaNW + lumaSW) - (lumaNE + lumaSE));
            const float dirReduce = max_f((lumaNW + lumaNE + lumaSW + lumaSE) * (0.25f * REDUCE_MUL), REDUCE_MIN);
            const float rcpDirMin = 1.0f / (min_f(fabsf(dirx), fabsf(diry)) + dirReduce);
            dirx = clampf(dirx * rcpDirMin, -SPAN_MAX, SPAN_MAX);
            diry = clampf(diry * rcpDirMin, -SPAN_MAX, SPAN_MAX);
            const float fx = (float)x, fy = (float)y;
            const Color rgbA1 = sample_f(src, W, H, fx + dirx * (1.0f / 3.0f - 0.5f), fy + diry * (1.0f / 3.0f - 0.5f));
            const Color rgbA2 = sample_f(src, W, H, fx + dirx * (2.0f / 3.0f - 0.5f), fy + diry * (2.0f / 3.0f - 0.5f));
            const Color rgbB1 = sample_f(src, W, H, fx + dirx * (0.0f / 3.0f - 0.5f), fy + diry * (0.0f / 3.0f - 0.5f));
            const Color rgbB2 = sample_f(src, W, H, fx + dirx * (3.0f / 3.0f - 0.5f), fy + diry * (3.0f / 3.0f - 0.5f));
            const Color rgbA = color_from_rgbaf(0.5f * ((float)rgbA1.r + (float)rgbA2.r), 0.5f * ((float)rgbA1.g + (float)rgbA2.g),
                                                0.5f * ((float)rgbA1.b + (float)rgbA2.b), 255.0f);
            const Color rgbB = color_from_rgbaf(0.5f * (float)rgbA.r + 0.25f * ((float)rgbB1.r + (float)rgbB2.r),
                                                0.5f * (float)rgbA.g + 0.25f * ((float)rgbB1.g + (float)rgbB2.g),
                                                0.5f * (float)rgbA.b + 0.25f * ((float)rgbB1.b + (float)rgbB2.b), 255.0f);
            const float lumaB = luma_from_color(rgbB);
            const int useA = lumaB < lumaMin || lumaB > lumaMax;
            dst[i] = useA ? rgbA : rgbB;
            if (branch) branch[i] = useA ? RFX_FXAA_RGBA : RFX_FXAA_RGBB;
        }
}

void rfx_spec_bright(const shs_canvas_spec_bright_desc *d, const float *spec01, uint8_t *dst8) {
    const int W = d->width, H = d->height;
    Color *dst = (Color *)dst8;
    const float gold[3] = {1.0f, 0.88f, 0.45f};
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const float s = spec01[i];
        float v = (s - d->threshold) / max_f(1e-6f, (1.0f - d->threshold));
        v = smoothstep01(v);
        v *= d->intensity;
        const float r = 255.0f * gold[0] * v, g = 255.0f * gold[1] * v, b = 255.0f * gold[2] * v;
        dst[i] = color_from_rgbaf(r, g, b, 255.0f);
    }
}

static Color mul_color(Color c, float k) {
    return (Color){(uint8_t)clampi(int_x86((float)c.r * k), 0, 255), (uint8_t)clampi(int_x86((float)c.g * k), 0, 255),
                   (uint8_t)clampi(int_x86((float)c.b * k), 0, 255), 255};
}

static Color add_color_clamped(Color a, Color b) {
    return (Color){(uint8_t)clampi((int)a.r + (int)b.r, 0, 255), (uint8_t)clampi((int)a.g + (int)b.g, 0, 255),
                   (uint8_t)clampi((int)a.b + (int)b.b, 0, 255), 255};
}

/* out may be base (hello_glowing_star.cpp:1310) */
void rfx_additive(int W, int H, const uint8_t *base8, const uint8_t *add8, float add_strength, uint8_t *out8) {
    const Color *base = (const Color *)base8, *add = (const Color *)add8;
    Color *out = (Color *)out8;
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const Color a = base[i];
        const Color b = mul_color(add[i], add_strength);
        out[i] = add_color_clamped(a, b);
    }
}

void rfx_lens_flare(const shs_canvas_lens_flare_desc *d, const uint8_t *src8, uint8_t *dst8, float *pq, int dbl, uint8_t *branch) {
    const int W = d->width, H = d->height, GHOSTS = d->n_ghosts;
    const Color *bright = (const Color *)src8;
    Color *dst = (Color *)dst8;
    const float intensity = d->intensity, halo_intensity = d->halo_intensity, chroma_shift_px = d->chroma_shift_px;
    const float cx = 0.5f * (float)W, cy = 0.5f * (float)H;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const float dx = (float)x - cx, dy = (float)y - cy;
            const float dist = sqrtf(dx * dx + dy * dy);
            const float nd = (dist / max_f(1.0f, min_f(cx, cy)));
            const float vign = 1.0f - smoothstep01(nd);
            float rr = 0, gg = 0, bb = 0;
            for (int k = 0; k < GHOSTS; ++k) {
                const float s = d->ghost_scales[k];
                const float sx = cx - dx * s, sy = cy - dy * s;
                float dirx = 0.0f, diry = 0.0f;
                if (dist > 1e-4f) {
                    dirx = dx / dist;
                    diry = dy / dist;
                }
                const Color cR = sample_f(bright, W, H, sx + dirx * chroma_shift_px, sy + diry * chroma_shift_px);
                const Color cG = sample_f(bright, W, H, sx, sy);
                const Color cB = sample_f(bright, W, H, sx - dirx * chroma_shift_px, sy - diry * chroma_shift_px);
                const float w = (0.45f + 0.55f * (1.0f - (float)k / (float)GHOSTS));
                rr += w * (float)cR.r;
                gg += w * (float)cG.g;
                bb += w * (float)cB.b;
            }
            {
                const float halo_scale = 0.35f;
                const float sx = cx - dx * halo_scale, sy = cy - dy * halo_scale;
                const Color hC = sample_f(bright, W, H, sx, sy);
                const float e = -8.0f * (nd - 0.35f) * (nd - 0.35f);
                const float ring = dbl ? (float)exp((double)e) : expf(e);
                rr += halo_intensity * ring * (float)hC.r;
                gg += halo_intensity * ring * (float)hC.g;
                bb += halo_intensity * ring * (float)hC.b;
            }
            rr *= intensity * vign;
            gg *= intensity * vign;
            bb *= intensity * vign;
            dst[i] = color_from_rgbaf(rr, gg, bb, 255.0f);
            if (pq) pq[4 * i] = rr, pq[4 * i + 1] = gg, pq[4 * i + 2] = bb, pq[4 * i + 3] = 1.0f;
            if (branch) branch[i] = (dist > 1e-4f) ? RFX_FLARE_OFF_CENTRE : RFX_FLARE_CENTRE;
        }
}
