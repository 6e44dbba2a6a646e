/*
 * ref_canvas_rt_pbr_soft.c -- TEST INFRASTRUCTURE ONLY: the C restatement of hello_pbr_light_shafts.cpp's camera pass
 * (PASS1) and its fragment shader, PBR under PCSS, the reference of tests/test_canvas_rt_pbr_soft*.py.  Nothing under
 * leisure-software-renderer_amd/ loads it.
 *
 * It restates, of the reference's cpp-folders/src/hello-render-target/hello_pbr_light_shafts.cpp:
 *   shadow_sample_depth_uv :579-588 over the legacy shs::ShadowMap::sample (hello-shs-renderer/shs_renderer.hpp:637-640,
 *   FLT_MAX outside -- the soft demo's file-local map clamps instead), POISSON_32 :591-625, hash_u32 / hash01 / rotate2
 *   :628-647, pcss_shadow_factor :650-762 with the constants :135-148, fragment_shader_pbr :768-850 and
 *   draw_triangle_tile_color_depth_motion :1015-1180 with its tile jobs.
 * What that file shares with hello_pbr.cpp text for text -- the PBR:: helpers :249-289, MaterialPBR / Uniforms, the
 * vertex shader, shadow_uvz_from_world :558-576, the raster but for fs(vin, px, py) -- and the IBL samplers of
 * shs/resources/ibl.hpp come from ../canvas_rt_pbr_ref/ref_canvas_rt_pbr.c, included below (which includes
 * ../canvas_rt_ref/ref_canvas_rt.c for the raster's shared pieces and PASS0).  The PCSS text is written again here from
 * the lines above, not taken from ../canvas_rt_soft_ref: test_canvas_rt_pbr_soft_ref.py pins one against the other.
 *
 * Every float operation rounds once (Makefile: no contraction, no fast math).  cosf, sinf, powf and lroundf are the
 * host libm's, as in the reference's build.  The demo needs SDL2, assimp and GLM and is not compiled anywhere in this
 * repository: this restatement is unpinned (README.md).
 */
#include "../canvas_rt_pbr_ref/ref_canvas_rt_pbr.c"

/* The constants of :135-148 (shs_rt_pcss has the same members). */
typedef struct {
    float light_uv_radius;
    float search_radius_texels;
    float min_filter_texels;
    float max_filter_texels;
    float epsilon;
    int32_t blocker_samples;
    int32_t pcf_samples;
} rps_pcss;

/* What happened inside one pcss_shadow_factor call (only the restatement records it). */
#define RPS_UV_OUTSIDE 1        /* the early 1.0: uv outside [0, 1] */
#define RPS_EMPTY_CENTRE 2      /* the early 1.0: the centre texel is empty */
#define RPS_NO_BLOCKER 4        /* blockerCnt <= 0 under a non-empty centre */
#define RPS_BLOCKER_OFF_MAP 8   /* a blocker tap fell outside [0, 1] */
#define RPS_BLOCKER_EMPTY 16    /* a blocker tap on the map read an empty texel */
#define RPS_PCF_OFF_MAP 32      /* a PCF tap fell outside [0, 1] */
#define RPS_PCF_EMPTY 64        /* a PCF tap on the map read an empty texel */
#define RPS_NOT_IN_LIGHT 128    /* no map, or shadow_uvz_from_world said no: pcss_shadow_factor was not called */
#define RPS_RADIUS_AT_MIN 256   /* clampf chose PCSS_MIN_FILTER_RADIUS_TEXELS */
#define RPS_RADIUS_AT_MAX 512   /* clampf chose PCSS_MAX_FILTER_RADIUS_TEXELS */
typedef struct {
    int32_t blockers;           /* blockerCnt, -1 when the search was not reached */
    float radius;               /* the clamped filterRadiusTex, -1 when it was not reached */
    int32_t flags;              /* RPS_* */
    float in[4];                /* uv.x, uv.y, z_receiver, bias as handed to pcss_shadow_factor (zeros: not called) */
} rps_debug;

/* shadow_sample_depth_uv :579-588 over shs::ShadowMap::sample (sm_sample of the shared file).  (int)lroundf(NaN) is
 * (int)LONG_MIN = 0 on x86-64. */
static float rps_sample_depth_uv(const float *sm, int w, int h, v2 uv) {
    if (uv.x < 0.0f || uv.x > 1.0f || uv.y < 0.0f || uv.y > 1.0f) return FLT_MAX;
    int x = (int)lroundf(uv.x * (float)(w - 1));
    int y = (int)lroundf(uv.y * (float)(h - 1));
    return sm_sample(sm, w, h, x, y);
}

/* POISSON_32 :591-625 */
static const v2 RPS_POISSON_32[32] = {
    {-0.613392f, 0.617481f},  {0.170019f, -0.040254f},  {-0.299417f, 0.791925f},  {0.645680f, 0.493210f},
    {-0.651784f, 0.717887f},  {0.421003f, 0.027070f},   {-0.817194f, -0.271096f}, {-0.705374f, -0.668203f},
    {0.977050f, -0.108615f},  {0.063326f, 0.142369f},   {0.203528f, 0.214331f},   {-0.667531f, 0.326090f},
    {-0.098422f, -0.295755f}, {-0.885922f, 0.215369f},  {0.566637f, 0.605213f},   {0.039766f, -0.396100f},
    {0.751946f, 0.453352f},   {0.078707f, -0.715323f},  {-0.075838f, -0.529344f}, {0.724479f, -0.580798f},
    {0.222999f, -0.215125f},  {-0.467574f, -0.405438f}, {-0.248268f, -0.814753f}, {0.354411f, -0.887570f},
    {0.175817f, 0.382366f},   {0.487472f, -0.063082f},  {-0.084078f, 0.898312f},  {0.488876f, -0.783441f},
    {0.470016f, 0.217933f},   {-0.696890f, -0.549791f}, {-0.149693f, 0.605762f},  {0.034211f, 0.979980f}};

/* hash_u32 / hash01 :628-641 */
static inline uint32_t rps_hash_u32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
static inline float rps_hash01(uint32_t x) { return (float)(rps_hash_u32(x) & 0x00FFFFFFu) / (float)0x01000000u; }

/* rotate2 :642-647 */
static inline v2 rps_rotate2(v2 p, float a) {
    float c = cosf(a);
    float s = sinf(a);
    v2 r = {c * p.x - s * p.y, s * p.x + c * p.y};
    return r;
}

static inline float rps_std_max(float a, float b) { return (a < b) ? b : a; }

/* pcss_shadow_factor :650-762 */
static float rps_pcss_shadow_factor(const float *sm, int w, int h, const rps_pcss *k, v2 uv, float z_receiver, float bias, int px, int py,
                                    rps_debug *dbg) {
    dbg->blockers = -1;
    dbg->radius = -1.0f;
    dbg->flags = 0;
    if (uv.x < 0.0f || uv.x > 1.0f || uv.y < 0.0f || uv.y > 1.0f) { dbg->flags |= RPS_UV_OUTSIDE; return 1.0f; }
    float centerDepth = rps_sample_depth_uv(sm, w, h, uv);
    if (centerDepth == FLT_MAX) { dbg->flags |= RPS_EMPTY_CENTRE; return 1.0f; }

    float texelSizeU = 1.0f / (float)w;
    float texelSizeV = 1.0f / (float)h;
    float searchRadiusTex = k->search_radius_texels;
    float searchRadiusU = searchRadiusTex * texelSizeU;
    float searchRadiusV = searchRadiusTex * texelSizeV;

    /* :676: '*' binds before '^', and an int times an unsigned is unsigned */
    uint32_t seed = (uint32_t)((uint32_t)px * 1973u ^ (uint32_t)py * 9277u ^ 0x9e3779b9u);
    float ang = rps_hash01(seed) * 6.2831853f;

    float blockerSum = 0.0f;
    int blockerCnt = 0;
    float zTest = z_receiver - bias;
    for (int i = 0; i < k->blocker_samples; ++i) {
        v2 o = RPS_POISSON_32[i & 31];
        o = rps_rotate2(o, ang);
        v2 suv = {uv.x + o.x * searchRadiusU, uv.y + o.y * searchRadiusV};
        float d = rps_sample_depth_uv(sm, w, h, suv);
        if (d == FLT_MAX) {
            dbg->flags |= (suv.x < 0.0f || suv.x > 1.0f || suv.y < 0.0f || suv.y > 1.0f) ? RPS_BLOCKER_OFF_MAP : RPS_BLOCKER_EMPTY;
            continue;
        }
        if (d < zTest) {
            blockerSum += d;
            blockerCnt++;
        }
    }
    dbg->blockers = blockerCnt;
    if (blockerCnt <= 0) { dbg->flags |= RPS_NO_BLOCKER; return 1.0f; }
    float avgBlocker = blockerSum / (float)blockerCnt;

    float zB = rps_std_max(k->epsilon, avgBlocker);
    float zR = rps_std_max(k->epsilon, z_receiver);
    float penumbraRatio = (zR - zB) / zB;
    penumbraRatio = rps_std_max(0.0f, penumbraRatio);

    float filterRadiusUvU = k->light_uv_radius * penumbraRatio;
    float filterRadiusUvV = k->light_uv_radius * penumbraRatio;
    float filterRadiusTexU = filterRadiusUvU / texelSizeU;
    float filterRadiusTexV = filterRadiusUvV / texelSizeV;
    float filterRadiusTex = 0.5f * (filterRadiusTexU + filterRadiusTexV);
    if (filterRadiusTex < k->min_filter_texels) dbg->flags |= RPS_RADIUS_AT_MIN;
    else if (filterRadiusTex > k->max_filter_texels) dbg->flags |= RPS_RADIUS_AT_MAX;
    filterRadiusTex = clampf(filterRadiusTex, k->min_filter_texels, k->max_filter_texels);
    dbg->radius = filterRadiusTex;
    filterRadiusUvU = filterRadiusTex * texelSizeU;
    filterRadiusUvV = filterRadiusTex * texelSizeV;

    float litSum = 0.0f;
    int litCnt = 0;
    float ang2 = rps_hash01(seed ^ 0xB5297A4Du) * 6.2831853f;
    for (int i = 0; i < k->pcf_samples; ++i) {
        v2 o = RPS_POISSON_32[i & 31];
        o = rps_rotate2(o, ang2);
        v2 suv = {uv.x + o.x * filterRadiusUvU, uv.y + o.y * filterRadiusUvV};
        float d = rps_sample_depth_uv(sm, w, h, suv);
        if (d == FLT_MAX) {
            dbg->flags |= (suv.x < 0.0f || suv.x > 1.0f || suv.y < 0.0f || suv.y > 1.0f) ? RPS_PCF_OFF_MAP : RPS_PCF_EMPTY;
            litSum += 1.0f;
            litCnt++;
            continue;
        }
        litSum += (z_receiver <= d + bias) ? 1.0f : 0.0f;
        litCnt++;
    }
    if (litCnt <= 0) return 1.0f;
    return litSum / (float)litCnt;
}

/* fragment_shader_pbr :768-850 with the base colour's bytes (of the texel or of mat.baseColor_srgb) given.  fr->pcf is
 * not read. */
static pbr_fragment rps_fragment_shader_pbr(const rcr_frame *fr, const rcp_consts *k, const rps_pcss *pk, const rcp_ibl *ibl,
                                            const rcp_material *mat, const uint8_t *base_srgb, v3 in_normal, v3 in_world_pos, int px,
                                            int py, rcp_debug *dbg, rps_debug *sdbg) {
    pbr_fragment f;
    v3 N = normalize3(in_normal);
    v3 cam = {fr->camera_pos[0], fr->camera_pos[1], fr->camera_pos[2]};
    v3 V = normalize3(sub3(cam, in_world_pos));
    v3 neg = {-fr->light_dir[0], -fr->light_dir[1], -fr->light_dir[2]};
    v3 L = normalize3(neg);
    v3 H = normalize3(add3(V, L));
    float NoV = g_max(0.0f, dot3(N, V));
    float NoL = g_max(0.0f, dot3(N, L));
    float NoH = g_max(0.0f, dot3(N, H));
    /* srgb_to_linear(color_to_rgb01(c)): pow(clamp(c / 255, 0, 1), 2.2) */
    v3 base;
    base.x = powf(g_clamp((float)base_srgb[0] / 255.0f, 0.0f, 1.0f), 2.2f);
    base.y = powf(g_clamp((float)base_srgb[1] / 255.0f, 0.0f, 1.0f), 2.2f);
    base.z = powf(g_clamp((float)base_srgb[2] / 255.0f, 0.0f, 1.0f), 2.2f);
    float metallic = saturate(mat->metallic);
    float roughness = clampf(mat->roughness, k->min_roughness, 1.0f);
    float ao = saturate(mat->ao);
    float om = 1.0f - metallic;
    v3 F0 = {0.04f * om + base.x * metallic, 0.04f * om + base.y * metallic, 0.04f * om + base.z * metallic};   /* glm::mix */
    v3 F = fresnel_schlick(F0, NoV);
    F.x *= 1.0f; F.y *= 0.96f; F.z *= 0.90f;
    v3 kd = {(1.0f - F.x) * (1.0f - metallic), (1.0f - F.y) * (1.0f - metallic), (1.0f - F.z) * (1.0f - metallic)};
    float alpha = roughness * roughness;
    float D = ndf_ggx(NoH, alpha);
    float G = g_smith(NoV, NoL, roughness, k->min_roughness);
    float ipi = 1.0f / PBR_PI;
    v3 direct_diffuse = {kd.x * base.x * ipi, kd.y * base.y * ipi, kd.z * base.z * ipi};
    float den4 = 4.0f * NoV * NoL;
    float den = g_max(1e-6f, den4);
    dbg->flags = (den == 1e-6f) ? RCP_DEN_CLAMPED : 0;
    float DG = D * G;
    v3 direct_specular = {DG * F.x / den, DG * F.y / den, DG * F.z / den};
    float I = k->direct_intensity;   /* direct_radiance = vec3(3.0f) :806 */
    v3 direct = {(direct_diffuse.x + direct_specular.x) * I * NoL, (direct_diffuse.y + direct_specular.y) * I * NoL,
                 (direct_diffuse.z + direct_specular.z) * I * NoL};
    float shadow = 1.0f;
    sdbg->blockers = -1;
    sdbg->radius = -1.0f;
    sdbg->flags = RPS_NOT_IN_LIGHT;
    memset(sdbg->in, 0, sizeof sdbg->in);
    if (fr->shadow) {
        v2 suv;
        float sz;
        if (shadow_uvz_from_world(fr->light_vp, in_world_pos, &suv, &sz)) {
            float slope = 1.0f - g_clamp(dot3(N, L), 0.0f, 1.0f);
            float bias = fr->bias_base + fr->bias_slope * slope;
            shadow = rps_pcss_shadow_factor(fr->shadow, fr->sw, fr->sh, pk, suv, sz, bias, px, py, sdbg);
            sdbg->in[0] = suv.x; sdbg->in[1] = suv.y; sdbg->in[2] = sz; sdbg->in[3] = bias;
        }
    }
    direct = scale3(direct, shadow);
    v3 ibl_c = {0.0f, 0.0f, 0.0f};
    dbg->face_n = dbg->face_r = dbg->m0 = dbg->m1 = -1;
    if (ibl && ibl->irr) {
        v3 irradiance = sample_cubemap(ibl->irr, ibl->irr_size, N, &dbg->face_n);
        float sd = saturate(mat->ibl_diffuse_intensity);
        v3 diffuseIBL = {irradiance.x * base.x * kd.x * sd, irradiance.y * base.y * kd.y * sd, irradiance.z * base.z * kd.z * sd};
        /* glm::reflect(-V, N): I - N * dot(N, I) * 2 */
        v3 Iv = {-V.x, -V.y, -V.z};
        float ni = dot3(N, Iv);
        v3 R = {Iv.x - N.x * ni * 2.0f, Iv.y - N.y * ni * 2.0f, Iv.z - N.z * ni * 2.0f};
        float lod = roughness * (float)(ibl->mip_count - 1);
        v3 prefiltered = sample_prefiltered(ibl, R, lod, &dbg->m0, &dbg->m1, &dbg->face_r);
        float ss = saturate(mat->ibl_specular_intensity) * saturate(mat->ibl_reflection_strength);
        v3 specIBL = {prefiltered.x * F.x * ss, prefiltered.y * F.y * ss, prefiltered.z * F.z * ss};
        ibl_c = add3(diffuseIBL, specIBL);
    }
    ibl_c = scale3(ibl_c, ao);
    v3 color = add3(direct, ibl_c);   /* :843: no minimum ambient in this demo */
    color = scale3(color, k->exposure);
    float c[3] = {color.x / (1.0f + color.x), color.y / (1.0f + color.y), color.z / (1.0f + color.z)};   /* tonemap_reinhard */
    for (int i = 0; i < 3; ++i) {
        f.prepow[i] = g_clamp(c[i], 0.0f, 1.0f);
        float s = powf(f.prepow[i], 1.0f / 2.2f);           /* linear_to_srgb */
        f.pre[i] = g_clamp(s, 0.0f, 1.0f) * 255.0f;         /* rgb01_to_color */
        f.rgba[i] = (uint8_t)f.pre[i];
    }
    f.pre[3] = shadow;
    f.rgba[3] = 255;
    return f;
}

/* The PCSS debug planes beside rcr_planes and rcp_debug_planes (canvas rows, any may be NULL). */
typedef struct {
    int32_t *blockers;
    float *radius;
    int32_t *pcss_flags;
    float *pcss_in;     /* 4 floats: uv.x, uv.y, z, bias handed to pcss_shadow_factor */
    int32_t *pxpy;      /* 2 ints: the screen pixel handed to the shader */
} rps_debug_planes;

/* draw_triangle_tile_color_depth_motion :1015-1180: hello_pbr.cpp's raster with fs(vin, px, py).  (The loop at
 * :1115-1120 has no side effect.) */
static void rps_draw_triangle_tile(const rcr_frame *fr, const rcp_consts *k, const rps_pcss *pk, const rcp_ibl *ibl, rcr_planes *t,
                                   const rcp_debug_planes *g, const rps_debug_planes *sg, const rcr_draw *u, const rcp_material *mat,
                                   const float *view_model, int32_t tri, const float *pos9, const float *nrm9, const float *uv6, int count,
                                   int tminx, int tminy, int tmaxx, int tmaxy) {
    const int W = fr->W, H = fr->H;
    varyings tri_in[3], poly[6];
    for (int i = 0; i < 3; ++i) {
        v3 p = {pos9[3 * i], pos9[3 * i + 1], pos9[3 * i + 2]}, n = {nrm9[3 * i], nrm9[3 * i + 1], nrm9[3 * i + 2]};
        v2 uv = {uv6 ? uv6[2 * i] : 0.0f, uv6 ? uv6[2 * i + 1] : 0.0f};
        tri_in[i] = vertex_shader_full(u, view_model, mat->normal_mat, p, n, uv);
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
                if (u->texels && u->tw > 0 && u->th > 0) {   /* sample_nearest_srgb */
                    texel = nearest_index(u->tw, u->th, in_uv);
                    base = u->texels + 4 * (size_t)texel;
                }
                rcp_debug dbg;
                rps_debug sdbg;
                pbr_fragment f = rps_fragment_shader_pbr(fr, k, pk, ibl, mat, base, in_normal, in_world, px, py, &dbg, &sdbg);
                memcpy(&t->color[o * 4], f.rgba, 4);
                if (t->prequant) memcpy(&t->prequant[o * 4], f.pre, sizeof f.pre);
                if (t->tri_id) t->tri_id[o] = id;
                if (t->texel) t->texel[o] = texel;
                if (t->flags) t->flags[o] = ((sdbg.flags & RPS_UV_OUTSIDE) ? RCR_PX_SUV_OUTSIDE : 0) | (area < 0 ? RCR_PX_NEG_AREA : 0);
                if (g) {
                    if (g->face_n) g->face_n[o] = dbg.face_n;
                    if (g->face_r) g->face_r[o] = dbg.face_r;
                    if (g->m0) g->m0[o] = dbg.m0;
                    if (g->m1) g->m1[o] = dbg.m1;
                    if (g->pbr_flags) g->pbr_flags[o] = dbg.flags;
                    if (g->prepow) memcpy(&g->prepow[o * 3], f.prepow, sizeof f.prepow);
                    if (g->frag_in) {
                        float *q = &g->frag_in[o * 6];
                        q[0] = in_normal.x; q[1] = in_normal.y; q[2] = in_normal.z;
                        q[3] = in_world.x; q[4] = in_world.y; q[5] = in_world.z;
                    }
                    if (g->base) memcpy(&g->base[o * 3], base, 3);
                }
                if (sg) {
                    if (sg->blockers) sg->blockers[o] = sdbg.blockers;
                    if (sg->radius) sg->radius[o] = sdbg.radius;
                    if (sg->pcss_flags) sg->pcss_flags[o] = sdbg.flags;
                    if (sg->pcss_in) memcpy(&sg->pcss_in[o * 4], sdbg.in, sizeof sdbg.in);
                    if (sg->pxpy) { sg->pxpy[o * 2] = px; sg->pxpy[o * 2 + 1] = py; }
                }
            }
        }
    }
}

/* hello_pbr_light_shafts.cpp's PASS1 without skybox_background_pass: the clear, then the camera pass's tile jobs.
 * mats[d] goes with draws[d].  Debug planes: -1 / 0 where nothing is shown. */
int rps_render(const rcr_frame *fr, const rcp_consts *k, const rps_pcss *pk, const rcp_ibl *ibl, const rcr_draw *draws,
               const rcp_material *mats, int n_draws, rcr_planes *t, const rcp_debug_planes *g, const rps_debug_planes *sg) {
    if (!fr || !k || !pk || !t || fr->W <= 0 || fr->H <= 0 || fr->tile_w <= 0 || fr->tile_h <= 0 || !t->color || !t->depth ||
        !t->velocity || n_draws < 0)
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
        if (g && g->face_n) g->face_n[i] = -1;
        if (g && g->face_r) g->face_r[i] = -1;
        if (g && g->m0) g->m0[i] = -1;
        if (g && g->m1) g->m1[i] = -1;
        if (g && g->pbr_flags) g->pbr_flags[i] = 0;
        if (sg && sg->blockers) sg->blockers[i] = -1;
        if (sg && sg->radius) sg->radius[i] = -1.0f;
        if (sg && sg->pcss_flags) sg->pcss_flags[i] = 0;
        if (sg && sg->pxpy) { sg->pxpy[i * 2] = -1; sg->pxpy[i * 2 + 1] = -1; }
    }
    if (t->prequant) memset(t->prequant, 0, sizeof(float) * 4 * npx);
    if (g && g->prepow) memset(g->prepow, 0, sizeof(float) * 3 * npx);
    if (g && g->frag_in) memset(g->frag_in, 0, sizeof(float) * 6 * npx);
    if (g && g->base) memset(g->base, 0, 3 * npx);
    if (sg && sg->pcss_in) memset(sg->pcss_in, 0, sizeof(float) * 4 * npx);
    memset(t->counters, 0, sizeof t->counters);
    const int cols = (W + fr->tile_w - 1) / fr->tile_w, rows = (H + fr->tile_h - 1) / fr->tile_h;
    for (int ty = 0; ty < rows; ty++) {
        for (int tx = 0; tx < cols; tx++) {
            const int tminx = tx * fr->tile_w, tminy = ty * fr->tile_h;
            const int tmaxx = ((tx + 1) * fr->tile_w < W ? (tx + 1) * fr->tile_w : W) - 1;
            const int tmaxy = ((ty + 1) * fr->tile_h < H ? (ty + 1) * fr->tile_h : H) - 1;
            int32_t tri = 0;
            for (int d = 0; d < n_draws; ++d) {
                float view_model[16];
                mat4_mul(fr->view, draws[d].model, view_model);   /* u.mv = view * model */
                for (int i = 0; i < draws[d].n_tris; ++i, ++tri)
                    rps_draw_triangle_tile(fr, k, pk, ibl, t, g, sg, &draws[d], &mats[d], view_model, tri,
                                           draws[d].positions + 9 * (size_t)i, draws[d].normals + 9 * (size_t)i,
                                           draws[d].uvs ? draws[d].uvs + 6 * (size_t)i : NULL, tx == 0 && ty == 0, tminx, tminy, tmaxx,
                                           tmaxy);
            }
        }
    }
    return 0;
}

/* ---- the pieces alone ---- */

/* fragment_shader_pbr for n fragments: normal3 / world3 the varyings, base3 the sRGB bytes, mats n materials, pxpy 2 n
 * screen pixels; pre4 (r, g, b) * 255 and the PCSS factor, prepow3 the colour before the final pow, rgba the bytes,
 * dbg5 (may be NULL) face_n, face_r, m0, m1, flags, sdbg3 (may be NULL) blockers, RPS_* flags and the radius' bits,
 * pcss_in4 (may be NULL) uv.x, uv.y, z, bias. */
int rps_fragments(const rcr_frame *fr, const rcp_consts *k, const rps_pcss *pk, const rcp_ibl *ibl, int n, const float *normal3,
                  const float *world3, const uint8_t *base3, const rcp_material *mats, const int32_t *pxpy, float *pre4, float *prepow3,
                  uint8_t *rgba, int32_t *dbg5, int32_t *sdbg3, float *pcss_in4) {
    if (!fr || !k || !pk || n < 0) return -1;
    for (int i = 0; i < n; ++i) {
        v3 nn = {normal3[3 * i], normal3[3 * i + 1], normal3[3 * i + 2]}, wp = {world3[3 * i], world3[3 * i + 1], world3[3 * i + 2]};
        rcp_debug dbg;
        rps_debug sdbg;
        pbr_fragment f = rps_fragment_shader_pbr(fr, k, pk, ibl, &mats[i], base3 + 3 * i, nn, wp, pxpy[2 * i], pxpy[2 * i + 1], &dbg, &sdbg);
        memcpy(pre4 + 4 * i, f.pre, sizeof f.pre);
        memcpy(prepow3 + 3 * i, f.prepow, sizeof f.prepow);
        memcpy(rgba + 4 * i, f.rgba, 4);
        if (dbg5) { dbg5[5 * i] = dbg.face_n; dbg5[5 * i + 1] = dbg.face_r; dbg5[5 * i + 2] = dbg.m0; dbg5[5 * i + 3] = dbg.m1; dbg5[5 * i + 4] = dbg.flags; }
        if (sdbg3) { sdbg3[3 * i] = sdbg.blockers; sdbg3[3 * i + 1] = sdbg.flags; memcpy(&sdbg3[3 * i + 2], &sdbg.radius, 4); }
        if (pcss_in4) memcpy(pcss_in4 + 4 * i, sdbg.in, sizeof sdbg.in);
    }
    return 0;
}
