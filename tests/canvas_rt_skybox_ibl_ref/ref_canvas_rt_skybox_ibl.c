/*
 * ref_canvas_rt_skybox_ibl.c -- TEST INFRASTRUCTURE ONLY: the C restatement of hello_ibl_skybox.cpp's camera pass, the
 * reference of tests/test_canvas_rt_skybox_ibl*.py.  Nothing under leisure-software-renderer_amd/ loads it.
 *
 * It restates, of the reference's cpp-folders/src/:
 *   hello-render-target/hello_ibl_skybox.cpp  fragment_shader_full :446-524 (Blinn-Phong under the 2x2-PCF shadow lookup,
 *       the ambient term tinted by u.sky->sample(N), a Schlick-weighted u.sky->sample(reflect(-V, N)) added), the raster
 *       that calls it (draw_triangle_tile_color_depth_motion_shadow :705-860, hello_shadow_mapping.cpp's :854-1022 apart
 *       from formatting) and its tile jobs; the knobs of Uniforms :336-339;
 *   hello-shs-renderer/shs_renderer.hpp  Math::clamp / saturate :130-145, Math::schlick_fresnel :164-169;
 *   GLM  glm::reflect (detail/func_geometric.inl): I - N * dot(N, I) * 2; glm::mix: x * (1 - a) + y * a.
 *
 * The raster's pieces and the hard demo's shadow helpers (the same text in hello_ibl_skybox.cpp :381-440) are
 * ../canvas_rt_ref/ref_canvas_rt.c's; the sky models and skybox_background_pass (:532-611, the clamp encode) are
 * ../canvas_rt_sky_ref/ref_canvas_rt_sky.c's, included below -- it includes the raster's file itself (through
 * ../canvas_rt_pbr_ref/ref_canvas_rt_pbr.c), so that one is not included a second time here.
 *
 * Every float operation rounds once (Makefile: no contraction, no fast math), in GLM's operation order.  powf, lroundf
 * and floorf are the host libm's, as in the reference's build.  The demo needs SDL2, assimp and GLM and is not
 * compiled anywhere in this repository: this restatement is unpinned (README.md).
 */
#include "../canvas_rt_sky_ref/ref_canvas_rt_sky.c"

/* The per-object knobs beside rcr_draw (shs_rt_skybox_ibl_draw has the same members). */
typedef struct {
    float ibl_ambient, ibl_refl, ibl_f0, ibl_refl_mix;
} rsi_knobs;

/* What one fragment did (only the restatement records it). */
typedef struct {
    int32_t branch_n, branch_r;   /* rsk_debug::branch of the two samples (cubemap: the face), -2 without a sky */
    float fresnel;                /* F */
    float env_n[3], env_r[3];     /* envN, envR */
    float refl_dir[3];            /* R (zeros without a sky) */
} rsi_debug;

typedef struct {
    float pre[4];    /* (r, g, b) * 255 before the truncation, shadow factor */
    uint8_t rgba[4];
} ibl_fragment;

/* Math::clamp :130-132 */
static inline float math_clamp(float v, float lo, float hi) { return (v < lo) ? lo : (v > hi ? hi : v); }

/* Math::schlick_fresnel :164-169 */
static inline float schlick_fresnel(float F0, float NoV) {
    float x = 1.0f - math_clamp(NoV, 0.0f, 1.0f);
    float x2 = x * x;
    float x5 = x2 * x2 * x;
    return F0 + (1.0f - F0) * x5;
}

/* glm::reflect */
static inline v3 reflect3(v3 I, v3 N) { return sub3(I, scale3(scale3(N, dot3(N, I)), 2.0f)); }

static inline int sky_bound(const rsk_sky *sky) { return sky && (sky->model == RSK_ANALYTIC || sky->model == RSK_CUBEMAP); }

/* fragment_shader_full :446-524 with the base colour's bytes (of the texel or of u.base_color) given; sky NULL (or of no
 * model): u.sky == nullptr */
static ibl_fragment fragment_shader_ibl(const rcr_frame *fr, const rsk_sky *sky, const rsi_knobs *k, const uint8_t *base, v3 in_normal,
                                        v3 in_world_pos, rsi_debug *dbg) {
    ibl_fragment f;
    v3 N = normalize3(in_normal);
    v3 neg = {-fr->light_dir[0], -fr->light_dir[1], -fr->light_dir[2]};
    v3 L = normalize3(neg);
    v3 cam = {fr->camera_pos[0], fr->camera_pos[1], fr->camera_pos[2]};
    v3 V = normalize3(sub3(cam, in_world_pos));
    float ambientStrength = 0.18f;
    float diff = g_max(dot3(N, L), 0.0f);
    v3 diffuse = {diff * 1.0f, diff * 1.0f, diff * 1.0f};
    v3 H = normalize3(add3(L, V));
    float spec = powf(g_max(dot3(N, H), 0.0f), 64.0f);   /* glm::pow */
    float sp = (0.45f * spec) * 1.0f;
    v3 specular = {sp, sp, sp};
    v3 baseColor = {(float)base[0] / 255.0f, (float)base[1] / 255.0f, (float)base[2] / 255.0f};   /* color_to_rgb01 */
    float shadow = 1.0f;
    if (fr->shadow) {
        v2 suv;
        float sz;
        if (shadow_uvz_from_world(fr->light_vp, in_world_pos, &suv, &sz)) {
            float slope = 1.0f - g_clamp(dot3(N, L), 0.0f, 1.0f);
            float bias = fr->bias_base + fr->bias_slope * slope;
            shadow = shadow_factor_pcf_2x2(fr->shadow, fr->sw, fr->sh, fr->pcf, suv, sz, bias);
        }
    }
    v3 envN = {1.0f, 1.0f, 1.0f};
    v3 envR = {0.0f, 0.0f, 0.0f};
    v3 R = {0.0f, 0.0f, 0.0f};
    dbg->branch_n = dbg->branch_r = -2;
    if (sky_bound(sky)) {
        rsk_debug g;
        envN = sky_sample(sky, N, &g);
        dbg->branch_n = g.branch;
        v3 negV = {-V.x, -V.y, -V.z};
        R = reflect3(negV, N);
        envR = sky_sample(sky, R, &g);
        dbg->branch_r = g.branch;
    }
    v3 one = {1.0f, 1.0f, 1.0f};
    v3 ambient = scale3(mix3(one, envN, saturate(k->ibl_ambient)), ambientStrength);   /* (a scalar times a vector: one product each) */
    float NoV = g_max(0.0f, dot3(N, V));
    float F = schlick_fresnel(k->ibl_f0, NoV);
    v3 refl = scale3(envR, (F * saturate(k->ibl_refl)) * saturate(k->ibl_refl_mix));
    v3 db = {diffuse.x * baseColor.x, diffuse.y * baseColor.y, diffuse.z * baseColor.z};
    v3 direct = scale3(add3(db, specular), shadow);
    v3 amb = {ambient.x * baseColor.x, ambient.y * baseColor.y, ambient.z * baseColor.z};
    v3 result = add3(add3(amb, direct), refl);
    result.x = g_clamp(result.x, 0.0f, 1.0f);
    result.y = g_clamp(result.y, 0.0f, 1.0f);
    result.z = g_clamp(result.z, 0.0f, 1.0f);
    /* rgb01_to_color: its own clamp changes nothing */
    f.pre[0] = g_clamp(result.x, 0.0f, 1.0f) * 255.0f;
    f.pre[1] = g_clamp(result.y, 0.0f, 1.0f) * 255.0f;
    f.pre[2] = g_clamp(result.z, 0.0f, 1.0f) * 255.0f;
    f.pre[3] = shadow;
    f.rgba[0] = (uint8_t)f.pre[0];
    f.rgba[1] = (uint8_t)f.pre[1];
    f.rgba[2] = (uint8_t)f.pre[2];
    f.rgba[3] = 255;
    dbg->fresnel = F;
    dbg->env_n[0] = envN.x; dbg->env_n[1] = envN.y; dbg->env_n[2] = envN.z;
    dbg->env_r[0] = envR.x; dbg->env_r[1] = envR.y; dbg->env_r[2] = envR.z;
    dbg->refl_dir[0] = R.x; dbg->refl_dir[1] = R.y; dbg->refl_dir[2] = R.z;
    return f;
}

/* Per-pixel planes only the restatement has (canvas rows, y * W + x); any may be NULL. */
typedef struct {
    int32_t *branch_n, *branch_r;   /* -2 where nothing is shown or no sky is bound */
    float *fresnel;
    float *env;                     /* 6 floats: envN, envR */
} rsi_debug_planes;

/* draw_triangle_tile_color_depth_motion_shadow :705-860: the hard demo's raster with this demo's fragment shader */
static void draw_triangle_tile_ibl(const rcr_frame *fr, const rsk_sky *sky, rcr_planes *t, const rsi_debug_planes *g, const rcr_draw *u,
                                   const rsi_knobs *k, const float *view_model, const float *n3, int32_t tri, const float *pos9,
                                   const float *nrm9, const float *uv6, int count, int tminx, int tminy, int tmaxx, int tmaxy) {
    const int W = fr->W, H = fr->H;
    varyings tri_in[3], poly[6];
    for (int i = 0; i < 3; ++i) {
        v3 p = {pos9[3 * i], pos9[3 * i + 1], pos9[3 * i + 2]}, n = {nrm9[3 * i], nrm9[3 * i + 1], nrm9[3 * i + 2]};
        v2 uv = {uv6 ? uv6[2 * i] : 0.0f, uv6 ? uv6[2 * i + 1] : 0.0f};
        tri_in[i] = vertex_shader_full(u, view_model, n3, p, n, uv);
    }
    const int n_poly = clip_poly_near_z(tri_in, 3, poly);
    if (count) {
        t->counters[0]++;
        if (n_poly == 3) t->counters[1]++;
        if (n_poly == 4) t->counters[2]++;
    }
    if (n_poly < 3) return;
    for (int ti = 1; ti + 1 < n_poly; ++ti) {
        const varyings tv[3] = {poly[0], poly[ti], poly[ti + 1]};
        const int32_t id = 2 * tri + (ti - 1);
        v3 sc3[3];
        int skip = 0;
        for (int i = 0; i < 3; ++i) {
            if (tv[i].position.w <= 1e-6f) { skip = 1; break; }
            sc3[i] = clip_to_screen(tv[i].position, W, H);
        }
        if (skip) continue;
        v2 v2d[3] = {{sc3[0].x, sc3[0].y}, {sc3[1].x, sc3[1].y}, {sc3[2].x, sc3[2].y}};
        v2 bboxmin, bboxmax;
        const int nonempty = tile_bbox(v2d, tminx, tminy, tmaxx, tmaxy, &bboxmin, &bboxmax);
        float area = (v2d[1].x - v2d[0].x) * (v2d[2].y - v2d[0].y) - (v2d[1].y - v2d[0].y) * (v2d[2].x - v2d[0].x);
        if (count && !(fabsf(area) < 1e-8f)) t->counters[3]++;
        if (!nonempty) continue;
        if (fabsf(area) < 1e-8f) continue;
        for (int px = (int)bboxmin.x; px <= (int)bboxmax.x; px++) {
            for (int py = (int)bboxmin.y; py <= (int)bboxmax.y; py++) {
                v2 P = {(float)px + 0.5f, (float)py + 0.5f};
                v3 bc = barycentric_coordinate(P, v2d);
                if (bc.x < 0 || bc.y < 0 || bc.z < 0) continue;
                float vz = bc.x * tv[0].view_z + bc.y * tv[1].view_z + bc.z * tv[2].view_z;
                int yc = (H - 1) - py;
                if (px < 0 || px >= W || yc < 0 || yc >= H) continue;
                const size_t o = (size_t)yc * W + px;
                if (!(vz < t->depth[o])) continue;
                t->depth[o] = vz;
                float w0 = tv[0].position.w, w1 = tv[1].position.w, w2 = tv[2].position.w;
                float invw0 = (fabsf(w0) < 1e-6f) ? 0.0f : 1.0f / w0;
                float invw1 = (fabsf(w1) < 1e-6f) ? 0.0f : 1.0f / w1;
                float invw2 = (fabsf(w2) < 1e-6f) ? 0.0f : 1.0f / w2;
                float invw_sum = bc.x * invw0 + bc.y * invw1 + bc.z * invw2;
                if (invw_sum <= 1e-8f) continue;
                v4 position = add4(add4(scale4(tv[0].position, bc.x), scale4(tv[1].position, bc.y)), scale4(tv[2].position, bc.z));
                v4 prev_position = add4(add4(scale4(tv[0].prev_position, bc.x), scale4(tv[1].prev_position, bc.y)),
                                        scale4(tv[2].prev_position, bc.z));
                v3 in_normal = normalize3(add3(add3(scale3(tv[0].normal, bc.x), scale3(tv[1].normal, bc.y)), scale3(tv[2].normal, bc.z)));
                v3 wp_over_w = add3(add3(scale3(scale3(tv[0].world_pos, invw0), bc.x), scale3(scale3(tv[1].world_pos, invw1), bc.y)),
                                    scale3(scale3(tv[2].world_pos, invw2), bc.z));
                v3 in_world = div3(wp_over_w, invw_sum);
                v2 uv_over_w;
                uv_over_w.x = (bc.x * (tv[0].uv.x * invw0) + bc.y * (tv[1].uv.x * invw1)) + bc.z * (tv[2].uv.x * invw2);
                uv_over_w.y = (bc.x * (tv[0].uv.y * invw0) + bc.y * (tv[1].uv.y * invw1)) + bc.z * (tv[2].uv.y * invw2);
                v2 in_uv = {uv_over_w.x / invw_sum, uv_over_w.y / invw_sum};
                v3 curr_s = clip_to_screen(position, W, H);
                v3 prev_s = clip_to_screen(prev_position, W, H);
                v2 v_screen = {curr_s.x - prev_s.x, curr_s.y - prev_s.y};
                v2 v_canvas = {v_screen.x, -v_screen.y};
                float len = sqrtf(dot2(v_canvas, v_canvas));
                if (len > fr->max_velocity_px && len > 1e-6f) {
                    float s = fr->max_velocity_px / len;
                    v_canvas.x *= s; v_canvas.y *= s;
                }
                t->velocity[o * 2 + 0] = v_canvas.x;
                t->velocity[o * 2 + 1] = v_canvas.y;
                int32_t texel = -1;
                const uint8_t *base = u->base_color;
                if (u->texels && u->tw > 0 && u->th > 0) {   /* sample_nearest (shs_renderer.hpp:367-377) */
                    texel = nearest_index(u->tw, u->th, in_uv);
                    base = u->texels + 4 * (size_t)texel;
                }
                rsi_debug dbg;
                ibl_fragment f = fragment_shader_ibl(fr, sky, k, base, in_normal, in_world, &dbg);
                memcpy(&t->color[o * 4], f.rgba, 4);
                if (t->prequant) memcpy(&t->prequant[o * 4], f.pre, sizeof f.pre);
                if (t->tri_id) t->tri_id[o] = id;
                if (t->texel) t->texel[o] = texel;
                if (t->flags) t->flags[o] = (area < 0 ? RCR_PX_NEG_AREA : 0);
                if (g) {
                    if (g->branch_n) g->branch_n[o] = dbg.branch_n;
                    if (g->branch_r) g->branch_r[o] = dbg.branch_r;
                    if (g->fresnel) g->fresnel[o] = dbg.fresnel;
                    if (g->env) { memcpy(&g->env[o * 6], dbg.env_n, sizeof dbg.env_n); memcpy(&g->env[o * 6 + 3], dbg.env_r, sizeof dbg.env_r); }
                }
            }
        }
    }
}

/* hello_ibl_skybox.cpp's camera pass without skybox_background_pass: the clear, then the tile jobs.  knobs[d] goes with
 * draws[d]; sky NULL: u.sky == nullptr. */
int rsi_render(const rsk_sky *sky, const rcr_frame *fr, const rcr_draw *draws, const rsi_knobs *knobs, int n_draws, rcr_planes *t,
               const rsi_debug_planes *g) {
    if (!fr || !t || fr->W <= 0 || fr->H <= 0 || fr->tile_w <= 0 || fr->tile_h <= 0 || !t->color || !t->depth || !t->velocity ||
        n_draws < 0 || (n_draws > 0 && (!draws || !knobs)))
        return -1;
    const int W = fr->W, H = fr->H;
    const size_t npx = (size_t)W * H;
    for (size_t i = 0; i < npx; ++i) {
        memcpy(&t->color[i * 4], fr->clear, 4);
        t->depth[i] = FLT_MAX;
        t->velocity[i * 2] = 0.0f; t->velocity[i * 2 + 1] = 0.0f;
        if (t->tri_id) t->tri_id[i] = -1;
        if (t->texel) t->texel[i] = -1;
        if (t->flags) t->flags[i] = 0;
        if (g && g->branch_n) g->branch_n[i] = -2;
        if (g && g->branch_r) g->branch_r[i] = -2;
        if (g && g->fresnel) g->fresnel[i] = 0.0f;
    }
    if (t->prequant) memset(t->prequant, 0, sizeof(float) * 4 * npx);
    if (g && g->env) memset(g->env, 0, sizeof(float) * 6 * npx);
    memset(t->counters, 0, sizeof t->counters);
    const int cols = (W + fr->tile_w - 1) / fr->tile_w, rows = (H + fr->tile_h - 1) / fr->tile_h;
    for (int ty = 0; ty < rows; ty++) {
        for (int tx = 0; tx < cols; tx++) {
            const int tminx = tx * fr->tile_w, tminy = ty * fr->tile_h;
            const int tmaxx = ((tx + 1) * fr->tile_w < W ? (tx + 1) * fr->tile_w : W) - 1;
            const int tmaxy = ((ty + 1) * fr->tile_h < H ? (ty + 1) * fr->tile_h : H) - 1;
            int32_t tri = 0;
            for (int d = 0; d < n_draws; ++d) {
                float view_model[16], inv[16], n3[9];
                mat4_mul(fr->view, draws[d].model, view_model);
                mat4_inverse(draws[d].model, inv);
                for (int c = 0; c < 3; ++c)          /* mat3(transpose(inv))[c][r] = inv[r][c] */
                    for (int r = 0; r < 3; ++r) n3[c * 3 + r] = inv[r * 4 + c];
                for (int i = 0; i < draws[d].n_tris; ++i, ++tri)
                    draw_triangle_tile_ibl(fr, sky, t, g, &draws[d], &knobs[d], view_model, n3, tri, draws[d].positions + 9 * (size_t)i,
                                           draws[d].normals + 9 * (size_t)i, draws[d].uvs ? draws[d].uvs + 6 * (size_t)i : NULL,
                                           tx == 0 && ty == 0, tminx, tminy, tmaxx, tmaxy);
            }
        }
    }
    return 0;
}

/* The demo's PASS1 with its background (:1106-1530 draws the sky first and the triangles over it): rsi_render, then the
 * sky, where one is bound, wherever no fragment is shown (t->tri_id is needed). */
int rsi_render_frame(const rsk_sky *sky, const rcr_frame *fr, const rcr_draw *draws, const rsi_knobs *knobs, int n_draws, rcr_planes *t,
                     const rsi_debug_planes *g) {
    if (!t || !t->tri_id) return -1;
    int rc = rsi_render(sky, fr, draws, knobs, n_draws, t, g);
    if (rc || !sky_bound(sky)) return rc;
    return rsk_compose(sky, fr->W, fr->H, t->tri_id, t->color, t->prequant, NULL, NULL, NULL);
}

/* ---- the pieces alone ---- */

/* fragment_shader_full for n fragments: normal3 / world3 the varyings, base3 the base colour's bytes, knobs n of them;
 * pre4 (r, g, b) * 255 and the shadow factor, rgba the bytes, dbg (may be NULL) n rsi_debug. */
int rsi_fragments(const rsk_sky *sky, const rcr_frame *fr, int n, const float *normal3, const float *world3, const uint8_t *base3,
                  const rsi_knobs *knobs, float *pre4, uint8_t *rgba, rsi_debug *dbg) {
    if (!fr || n < 0) return -1;
    for (int i = 0; i < n; ++i) {
        v3 nn = {normal3[3 * i], normal3[3 * i + 1], normal3[3 * i + 2]}, wp = {world3[3 * i], world3[3 * i + 1], world3[3 * i + 2]};
        rsi_debug d;
        ibl_fragment f = fragment_shader_ibl(fr, sky, &knobs[i], base3 + 3 * i, nn, wp, &d);
        memcpy(pre4 + 4 * i, f.pre, sizeof f.pre);
        memcpy(rgba + 4 * i, f.rgba, 4);
        if (dbg) dbg[i] = d;
    }
    return 0;
}

float rsi_schlick_fresnel(float f0, float nov) { return schlick_fresnel(f0, nov); }

size_t rsi_sizeof_knobs(void) { return sizeof(rsi_knobs); }
size_t rsi_sizeof_debug(void) { return sizeof(rsi_debug); }
