// shs_canvas_rt_shaders.hpp -- the fragment shaders of the Canvas render-target raster's camera pass, one per
// shading (shs_canvas_rt.hip's header comment lists the demos and what "soft :line", "pbr :line", "shafts :line",
// "ibl :line", "water :line" and "sky :line" cite), each with the samplers only it and its *_samples kernel read.
// Every shader starts with the front end of shs_canvas_rt_frag.hpp -- the fragment's inputs, the velocity, the world
// position, the normal, the base colour, the shadow lookup -- and then has only its own lighting.  Included by
// shs_canvas_rt.hip alone.
#pragma once
#include "shs_canvas_rt_frag.hpp"

namespace shs_dev {
namespace {

// The shown fragment of a camera-pass pixel (:971-1013) at the shading sub-triangle's barycentrics, through
// fragment_shader_full :699-750.
__device__ void shade_pixel(const RtParams &p, int32_t id, float u, float v, float w, uint32_t &rgba, float2 &vel, float4 &pq) {
    const Frag f(p, id, u, v, w);
    vel = frag_velocity(p, f.y, u, v, w);
    const f3 wp = f.world();
    const f3 N = f.normal();
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    const float ambient = 0.18f * 1.0f;
    const float ndotl = dot3(N, L);
    const float diffuse = g_max(ndotl, 0.0f) * 1.0f;
    const f3 H = normalize3(add3(L, V));
    const float spec = pow64(g_max(dot3(N, H), 0.0f));
    const float specular = (0.45f * spec) * 1.0f;
    const f3 base = frag_base01(f);
    float shadow = 1.0f;
    if (p.shadow) shadow = shadow_factor(p, wp, ndotl);
    const float lit = ambient + shadow * (diffuse + specular);
    const float pr = g_clamp01(lit * base.x) * 255, pg = g_clamp01(lit * base.y) * 255, pb = g_clamp01(lit * base.z) * 255;
    rgba = pack_rgba(pr, pg, pb);
    pq = make_float4(pr, pg, pb, shadow);
}

// The shown fragment of hello_shadow_mapping_soft.cpp's camera pass (soft :961-979) at screen pixel (px, py):
// the same interpolation without position / prev_position (that demo has no motion buffer), then
// fragment_shader_softshadow (soft :991-1040) -- not the hard shader with other constants: the ambient and the
// diffuse term are multiplied by the base colour, the specular term is not.
__device__ void shade_pixel_soft(const RtParams &p, int32_t id, float u, float v, float w, int px, int py, uint32_t &rgba, float4 &pq) {
    const Frag f(p, id, u, v, w);
    const f3 wp = f.world();
    const f3 N = f.normal();
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    const f3 base = frag_base01(f);
    const float ndotl = dot3(N, L);
    const float diffuse = g_max(ndotl, 0.0f) * 1.0f;
    const f3 H = normalize3(add3(L, V));
    const float spec = pow64(g_max(dot3(N, H), 0.0f));
    const float specular = (0.45f * spec) * 1.0f;
    float shadow = 1.0f;
    if (p.shadow) shadow = pcss_from_world(p, wp, ndotl, px, py);
    // amb = 0.22 * baseColor; direct = shadow * (diffuse * baseColor + specular); clamp(amb + direct)
    const float pr = g_clamp01(0.22f * base.x + shadow * (diffuse * base.x + specular)) * 255;
    const float pg = g_clamp01(0.22f * base.y + shadow * (diffuse * base.y + specular)) * 255;
    const float pb = g_clamp01(0.22f * base.z + shadow * (diffuse * base.z + specular)) * 255;
    rgba = pack_rgba(pr, pg, pb);
    pq = make_float4(pr, pg, pb, shadow);
}

// ---- hello_pbr.cpp: image-based lighting and the GGX fragment shader ("pbr :line") ------------------

// sample_face_bilinear_linear_vec (shs/resources/ibl.hpp:215-234) over a level of the IBL allocation (RtParams::ibl).
// std::clamp keeps a NaN; (int)std::floor is the x86-64 conversion, so a NaN coordinate reads texel 0 and 1.
__device__ f3 ibl_sample_face(const float4 *ibl, int first, int size, int face, float u, float v) {
    u = (u < 0.0f) ? 0.0f : (1.0f < u ? 1.0f : u);
    v = (v < 0.0f) ? 0.0f : (1.0f < v ? 1.0f : v);
    const float fx = u * (float)(size - 1);
    const float fy = v * (float)(size - 1);
    const int x0 = clampi(int_x86(floorf(fx)), 0, size - 1);
    const int y0 = clampi(int_x86(floorf(fy)), 0, size - 1);
    const int x1 = clampi(x0 + 1, 0, size - 1);
    const int y1 = clampi(y0 + 1, 0, size - 1);
    const float tx = fx - (float)x0;
    const float ty = fy - (float)y0;
    const float4 *f = ibl + first + (size_t)face * size * size;
    const float4 c00 = f[y0 * size + x0], c10 = f[y0 * size + x1], c01 = f[y1 * size + x0], c11 = f[y1 * size + x1];
    // glm::mix(x, y, a): x * (1 - a) + y * a
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    const f3 cx0 = {c00.x * ux + c10.x * tx, c00.y * ux + c10.y * tx, c00.z * ux + c10.z * tx};
    const f3 cx1 = {c01.x * ux + c11.x * tx, c01.y * ux + c11.y * tx, c01.z * ux + c11.z * tx};
    return {cx0.x * uy + cx1.x * ty, cx0.y * uy + cx1.y * ty, cx0.z * uy + cx1.z * ty};
}

// sample_cubemap_linear_vec (ibl.hpp:236-270) of level `level` (0: irradiance, 1 + m: specular mip m)
__device__ f3 ibl_sample_cube(const float4 *ibl, int level, f3 d) {
    const int4 hd = reinterpret_cast<const int4 *>(ibl)[level];   // {first texel, size}
    const float len = sqrtf(dot3(d, d));
    if (len < 1e-8f) return {0.0f, 0.0f, 0.0f};
    d = {d.x / len, d.y / len, d.z / len};
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int face;
    float u, v;
    if (ax >= ay && ax >= az) {
        if (d.x > 0.0f) { face = 0; u = -d.z / ax; v = d.y / ax; }
        else            { face = 1; u = d.z / ax; v = d.y / ax; }
    } else if (ay >= ax && ay >= az) {
        if (d.y > 0.0f) { face = 2; u = d.x / ay; v = -d.z / ay; }
        else            { face = 3; u = d.x / ay; v = d.z / ay; }
    } else {
        if (d.z > 0.0f) { face = 4; u = d.x / az; v = d.y / az; }
        else            { face = 5; u = -d.x / az; v = d.y / az; }
    }
    u = 0.5f * (u + 1.0f);
    v = 0.5f * (v + 1.0f);
    return ibl_sample_face(ibl, hd.x, hd.y, face, u, v);
}

// sample_prefiltered_spec_trilinear (ibl.hpp:272-286); a NaN lod passes std::clamp and converts to INT_MIN, whose
// mip index is clamped here (the reference would index out of its vector)
__device__ f3 ibl_sample_trilinear(const float4 *ibl, int mips, f3 d, float lod) {
    const float mmax = (float)(mips - 1);
    lod = (lod < 0.0f) ? 0.0f : (mmax < lod ? mmax : lod);
    const int m0 = clampi(int_x86(floorf(lod)), 0, mips - 1);
    const int m1 = min(m0 + 1, mips - 1);
    const float t = lod - (float)m0;
    const f3 c0 = ibl_sample_cube(ibl, 1 + m0, d);
    const f3 c1 = ibl_sample_cube(ibl, 1 + m1, d);
    const float s = 1.0f - t;
    return {c0.x * s + c1.x * t, c0.y * s + c1.y * t, c0.z * s + c1.z * t};
}

// One channel's way to the screen in hello_pbr.cpp (fragment_shader_pbr :722-726, skybox_background_pass :785-789):
// the exposure, tonemap_reinhard, linear_to_srgb, and rgb01_to_color up to the truncation: the channel * 255.
__device__ __forceinline__ float encode_reinhard(float x, float exposure) {
    x = x * exposure;
    x = x / (1.0f + x);                        // tonemap_reinhard
    x = powf(g_clamp01(x), 1.0f / 2.2f);       // linear_to_srgb
    return g_clamp01(x) * 255.0f;              // rgb01_to_color
}

// The shown fragment of hello_pbr.cpp's camera pass (pbr :986-1035, the hard demo's interpolation and velocity)
// through fragment_shader_pbr (pbr :627-727): Cook-Torrance GGX under the hard demo's shadow lookup, plus the
// irradiance and prefiltered-specular IBL.  The direct term is finished before the IBL gathers start.
// SOFT: hello_pbr_light_shafts.cpp's fragment_shader_pbr (shafts :768-850) at screen pixel (px, py) instead -- the same
// text but for the shadow factor, which is pcss_shadow_factor over the bias of shafts :814-815 (SHS_RT_PCF is not read),
// and the missing minimum ambient.  Its ShadowMap is the legacy one, FLT_MAX outside, where the soft demo's clamps:
// pcss_tap never looks outside.
template <bool SOFT>
__device__ void shade_pixel_pbr(const RtParams &p, int32_t id, float u, float v, float w, int px, int py, uint32_t &rgba, float2 &vel,
                                float4 &pq) {
    const Frag f(p, id, u, v, w);
    vel = frag_velocity(p, f.y, u, v, w);
    const f3 wp = f.world();
    const f3 N = f.normal();
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 H = normalize3(add3(V, L));
    const float ndotl = dot3(N, L);
    const float NoV = g_max(0.0f, dot3(N, V)), NoL = g_max(0.0f, ndotl), NoH = g_max(0.0f, dot3(N, H));
    const float4 m0 = reinterpret_cast<const float4 *>(&p.pbr_draws[f.r.draw])[0];   // base rgb, metallic
    const float4 m1 = reinterpret_cast<const float4 *>(&p.pbr_draws[f.r.draw])[1];   // roughness, ao, ibl diffuse, ibl specular
    f3 base = {m0.x, m0.y, m0.z};
    if (f.dr.texels) {
        // sample_nearest_srgb = sample_nearest (shs_renderer.hpp:367-381), then srgb_to_linear of the bytes
        const float2 t = f.uv();
        const uint32_t tc = sample_nearest_texel(f.dr, t.x, t.y);
        base = f3{p.srgb_lut[tc & 0xffu], p.srgb_lut[(tc >> 8) & 0xffu], p.srgb_lut[(tc >> 16) & 0xffu]};
    }
    const float metallic = m0.w, roughness = m1.x, ao = m1.y;
    const float om = 1.0f - metallic;
    const f3 F0 = {0.04f * om + base.x * metallic, 0.04f * om + base.y * metallic, 0.04f * om + base.z * metallic};
    // fresnel_schlick (pbr :242-249), then the blue attenuation
    const float fx = 1.0f - saturate(NoV);
    const float fx2 = fx * fx;
    const float fx5 = fx2 * fx2 * fx;
    const f3 Fr = {(F0.x + (1.0f - F0.x) * fx5) * 1.0f, (F0.y + (1.0f - F0.y) * fx5) * 0.96f, (F0.z + (1.0f - F0.z) * fx5) * 0.90f};
    const f3 kd = {(1.0f - Fr.x) * om, (1.0f - Fr.y) * om, (1.0f - Fr.z) * om};
    // ndf_ggx (:251-257), g_smith over g_schlick_ggx (:259-277; its second clamp of the roughness changes nothing)
    const float PI = 3.14159265358979323846f;
    const float alpha = roughness * roughness;
    const float sh = saturate(NoH);
    const float a2 = alpha * alpha;
    const float dd = (sh * sh) * (a2 - 1.0f) + 1.0f;
    const float D = a2 / (PI * dd * dd);
    const float r1 = roughness + 1.0f;
    const float k = (r1 * r1) / 8.0f;
    const float sv_ = saturate(NoV), sl_ = saturate(NoL);
    const float G = (sv_ / (sv_ * (1.0f - k) + k)) * (sl_ / (sl_ * (1.0f - k) + k));
    const float DG = D * G;
    const float den = g_max(1e-6f, 4.0f * NoV * NoL);
    float shadow = 1.0f;
    if (p.shadow) shadow = SOFT ? pcss_from_world(p, wp, ndotl, px, py) : shadow_factor(p, wp, ndotl);
    f3 c;
    {
        const float ipi = 1.0f / PI;
        const float I = p.pbr_intensity;
        c.x = ((((kd.x * base.x) * ipi + (DG * Fr.x) / den) * I) * NoL) * shadow;
        c.y = ((((kd.y * base.y) * ipi + (DG * Fr.y) / den) * I) * NoL) * shadow;
        c.z = ((((kd.z * base.z) * ipi + (DG * Fr.z) / den) * I) * NoL) * shadow;
    }
    f3 ibl = {0.0f, 0.0f, 0.0f};
    if (p.ibl) {
        const f3 irr = ibl_sample_cube(p.ibl, 0, N);
        const f3 R = reflect3(f3{-V.x, -V.y, -V.z}, N);
        const float lod = roughness * (float)(p.ibl_mips - 1);
        const f3 pre = ibl_sample_trilinear(p.ibl, p.ibl_mips, R, lod);
        ibl.x = ((irr.x * base.x) * kd.x) * m1.z + (pre.x * Fr.x) * m1.w;
        ibl.y = ((irr.y * base.y) * kd.y) * m1.z + (pre.y * Fr.y) * m1.w;
        ibl.z = ((irr.z * base.z) * kd.z) * m1.z + (pre.z * Fr.z) * m1.w;
    }
    float out[3] = {c.x + ibl.x * ao, c.y + ibl.y * ao, c.z + ibl.z * ao};
    const float bs[3] = {base.x, base.y, base.z};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float x = out[i];
        if constexpr (!SOFT) x = x + (bs[i] * 0.03f) * ao;   // the minimum ambient (hello_pbr.cpp alone)
        out[i] = encode_reinhard(x, p.pbr_exposure);
    }
    rgba = pack_rgba(out[0], out[1], out[2]);
    pq = make_float4(out[0], out[1], out[2], shadow);
}

// ---- the legacy sky models ("sky :line": hello-shs-renderer/shs_renderer.hpp), sampled by the background pass and by
// hello_ibl_skybox.cpp's shader -------------------------------------------------------------------------------

__device__ __forceinline__ f3 ld3(const float *p) { return {p[0], p[1], p[2]}; }

// AnalyticSky::sample (sky :558-608) after the host's part (RtSkyModel).  Its three std::pow(x, 3.0f / 4.0f / 12.0f)
// are products in double rounded once, as pow64; everything else is + - * / sqrt and compares, so cosGamma and with
// it the disc / edge branch are the reference's.
__device__ f3 sky_analytic(const RtSkyModel &m, f3 dir) {
    const f3 d = normalize3(dir);
    const f3 s = ld3(m.s);
    const float cosTheta = g_min(g_max(d.y, -1.0f), 1.0f);
    const float cosGamma = dot3(d, s);
    // glm::smoothstep(-0.15f, 0.15f, cosTheta)
    const float t = g_clamp01((cosTheta - -0.15f) / (0.15f - -0.15f));
    const float sky_ground = t * t * (3.0f - 2.0f * t);
    const double up = (double)(1.0f - g_max(0.0f, cosTheta));
    const f3 upper = mix3(ld3(m.zenith), ld3(m.horizon), (float)(up * up * up));
    const double hz = (double)(1.0f + g_min(0.0f, cosTheta)), hz2 = hz * hz;
    const f3 lower = mix3(ld3(m.ground), ld3(m.half_horizon), (float)(hz2 * hz2));
    f3 c = mix3(lower, upper, sky_ground);
    const double g = (double)g_clamp01(cosGamma), g2 = g * g, g4 = g2 * g2;
    const float glow = (float)((g4 * g4) * g4);
    c = add3(c, sc3(ld3(m.glow), glow));
    if (cosGamma > 0.9998f) {
        c = {4.0f, 3.5f, 3.0f};
    } else if (cosGamma > 0.9992f) {
        const float edge = (cosGamma - 0.9992f) / (0.9998f - 0.9992f);
        c = mix3(c, f3{3.0f, 2.5f, 1.5f}, edge);
    }
    return c;
}

// Texture2D::get (sky :360-363) then to_lin (sky :462-465): {0, 0, 0, 0} out of bounds, which the table takes to 0 as
// pow(0, 2.2f).  An unconditional load at a clamped address plus a select (as pcss_tap).
__device__ __forceinline__ f3 sky_texel(const uint32_t *tex, int w, int h, const float *lut, int x, int y) {
    const bool in = x >= 0 && x < w && y >= 0 && y < h;
    const uint32_t raw = tex[(size_t)clampi(y, 0, h - 1) * w + clampi(x, 0, w - 1)];
    const uint32_t tc = in ? raw : 0u;
    return {lut[tc & 0xffu], lut[(tc >> 8) & 0xffu], lut[(tc >> 16) & 0xffu]};
}

// CubeMapSky::sample over sample_face_bilinear (sky :439-512).  A NaN coordinate passes glm::clamp and converts to
// INT_MIN (x1 = INT_MIN + 1): all four texels are out of bounds.
__device__ f3 sky_cubemap(const RtSkyModel &m, f3 d) {
    const float len = sqrtf(dot3(d, d));
    if (len < 1e-8f) return {0.0f, 0.0f, 0.0f};
    d = {d.x / len, d.y / len, d.z / len};
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int face;
    float u, v;
    if (ax >= ay && ax >= az) {
        if (d.x > 0.0f) { face = 0; u = -d.z / ax; v = d.y / ax; }
        else            { face = 1; u = d.z / ax; v = d.y / ax; }
    } else if (ay >= ax && ay >= az) {
        if (d.y > 0.0f) { face = 2; u = d.x / ay; v = -d.z / ay; }
        else            { face = 3; u = d.x / ay; v = d.z / ay; }
    } else {
        if (d.z > 0.0f) { face = 4; u = d.x / az; v = d.y / az; }
        else            { face = 5; u = -d.x / az; v = d.y / az; }
    }
    u = 0.5f * (u + 1.0f);
    v = 0.5f * (v + 1.0f);
    // the face's texture out of the kernel arguments: selects over the six, not a per-lane index into them
    const uint32_t *tex = m.face[0];
    int w = m.fw[0], h = m.fh[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) {
        const bool is = face == k;
        tex = is ? m.face[k] : tex;
        w = is ? m.fw[k] : w;
        h = is ? m.fh[k] : h;
    }
    u = g_clamp01(u);   // glm::clamp: min(max(x, 0), 1)
    v = g_clamp01(v);
    const float fx = u * (float)(w - 1);
    const float fy = v * (float)(h - 1);
    const int x0 = int_x86(floorf(fx));
    const int y0 = int_x86(floorf(fy));
    const int x1 = min(x0 + 1, w - 1);
    const int y1 = min(y0 + 1, h - 1);
    const float tx = fx - (float)x0;
    const float ty = fy - (float)y0;
    const f3 v00 = sky_texel(tex, w, h, m.srgb_lut, x0, y0), v10 = sky_texel(tex, w, h, m.srgb_lut, x1, y0);
    const f3 v01 = sky_texel(tex, w, h, m.srgb_lut, x0, y1), v11 = sky_texel(tex, w, h, m.srgb_lut, x1, y1);
    const f3 vx0 = mix3(v00, v10, tx);
    const f3 vx1 = mix3(v01, v11, tx);
    return sc3(mix3(vx0, vx1, ty), m.intensity);
}

// AbstractSky::sample of the legacy sky models
template <int MODEL>
__device__ __forceinline__ f3 sky_sample(const RtSkyModel &m, f3 d) {
    if constexpr (MODEL == RT_SKY_CUBEMAP) return sky_cubemap(m, d);
    else return sky_analytic(m, d);
}

// ---- hello_ibl_skybox.cpp: the sky-lit Blinn-Phong fragment shader ("ibl :line") --------------------

// The shown fragment of hello_ibl_skybox.cpp's camera pass (ibl :810-852, the hard demo's interpolation and velocity)
// through its fragment_shader_full (ibl :446-524): the hard demo's Blinn-Phong under the same shadow lookup, with the
// ambient term tinted by u.sky->sample(N) and a Schlick-weighted u.sky->sample(reflect(-V, N)) added.  Not the hard
// shader plus two terms: the base colour multiplies the ambient and the diffuse term, not the specular one.
// SKY: u.sky, a compile-time choice (RT_SKY_NONE: u.sky == nullptr, envN = 1 and envR = 0; no gathers but the cubemap's).
// Everything of the direct term is reduced to seven floats (base, shadow, diffuse, specular, F) before the sky is
// sampled: N and V are all the two samples need.
template <int SKY>
__device__ void shade_pixel_ibl(const RtParams &p, int32_t id, float u, float v, float w, uint32_t &rgba, float2 &vel, float4 &pq) {
    const Frag f(p, id, u, v, w);
    vel = frag_velocity(p, f.y, u, v, w);
    const f3 wp = f.world();
    const f3 N = f.normal();
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    const float ndotl = dot3(N, L);
    const float diffuse = g_max(ndotl, 0.0f) * 1.0f;
    const f3 H = normalize3(add3(L, V));
    const float spec = pow64(g_max(dot3(N, H), 0.0f));
    const float specular = (0.45f * spec) * 1.0f;
    const f3 base = frag_base01(f);
    float shadow = 1.0f;
    if (p.shadow) shadow = shadow_factor(p, wp, ndotl);
    const float4 kn = *reinterpret_cast<const float4 *>(&p.ibl_draws[f.r.draw]);   // ambient, refl, f0, refl_mix
    // Math::schlick_fresnel(u.ibl_f0, max(0, N.V)) (shs_renderer.hpp:164-169)
    const float fx = 1.0f - saturate(g_max(0.0f, dot3(N, V)));
    const float fx2 = fx * fx;
    const float fx5 = fx2 * fx2 * fx;
    const float F = kn.z + (1.0f - kn.z) * fx5;
    const float rk = (F * kn.y) * kn.w;
    f3 envN = {1.0f, 1.0f, 1.0f}, envR = {0.0f, 0.0f, 0.0f};
    if constexpr (SKY != RT_SKY_NONE) {
        envN = sky_sample<SKY>(p.sky, N);
        envR = sky_sample<SKY>(p.sky, reflect3(f3{-V.x, -V.y, -V.z}, N));
    }
    // ambient = 0.18 * mix(vec3(1), envN, a); amb = ambient * base; direct = shadow * (diffuse * base + specular);
    // refl = envR * rk; clamp((amb + direct) + refl)
    const f3 tint = mix3(f3{1.0f, 1.0f, 1.0f}, envN, kn.x);
    const float pr = g_clamp01(((0.18f * tint.x) * base.x + shadow * (diffuse * base.x + specular)) + envR.x * rk) * 255;
    const float pg = g_clamp01(((0.18f * tint.y) * base.y + shadow * (diffuse * base.y + specular)) + envR.y * rk) * 255;
    const float pb = g_clamp01(((0.18f * tint.z) * base.z + shadow * (diffuse * base.z + specular)) + envR.z * rk) * 255;
    rgba = pack_rgba(pr, pg, pb);
    pq = make_float4(pr, pg, pb, shadow);
}

// ---- hello_ibl_skybox_optimized.cpp ("opt :line"; hello_ibl_skybox_xsimd.cpp carries the same text at :822-911): Blinn-Phong
// with a per-object exponent, lit by the irradiance cubemap and the prefiltered-specular mip chain -----------------

// glm::pow(x, shininess) with the exponent a per-draw datum: one double pow, rounded to float once.  The double
// result's error is some 2^-52 of its value, 2^28 times below half a float ulp, so the float is the correctly rounded
// power but where the exact value lies that close to a rounding boundary; the reference's powf is the host libm's, as
// close to correct.  pow(x, 0) is 1 for every x, a NaN included, and pow(0, s > 0) is 0, as powf has them.
__device__ __forceinline__ float pow_var(float x, float e) { return (float)pow((double)x, (double)e); }

// The shown fragment of the demo's camera pass (opt :1125-1291: the hard demo's raster, interpolation and velocity)
// through fragment_shader_full (opt :875-958): the hard demo's Blinn-Phong with the draw's shininess, the specular term
// not taking the base colour, under the hard demo's shadow lookup on the direct term alone; then the irradiance along N
// and the prefiltered specular along reflect(-V, N) at lod = sqrt(2 / (shininess + 2)) * (mips - 1), split by Schlick's F
// into kd = 1 - F and ks = F.  The file-local CubeMapF samplers (opt :246-330, :504-518) are ibl.hpp:215-286 but for
// Math::saturate where those have std::clamp, which keep a NaN alike: ibl_sample_cube / ibl_sample_trilinear.  The
// direct term and the shadow lookup are finished (amb + direct, three floats) before the IBL gathers start.
__device__ void shade_pixel_ibl_phong(const RtParams &p, int32_t id, float u, float v, float w, uint32_t &rgba, float2 &vel, float4 &pq) {
    const Frag f(p, id, u, v, w);
    vel = frag_velocity(p, f.y, u, v, w);
    const f3 wp = f.world();
    const f3 N = f.normal();
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    const float4 kn = reinterpret_cast<const float4 *>(&p.ibl_phong_draws[f.r.draw])[0];   // ambient, refl, f0, refl_mix
    const float4 ks = reinterpret_cast<const float4 *>(&p.ibl_phong_draws[f.r.draw])[1];   // shininess, rough
    const float ndotl = dot3(N, L);
    const float diffuse = g_max(ndotl, 0.0f) * 1.0f;
    const f3 H = normalize3(add3(L, V));
    const float spec = pow_var(g_max(dot3(N, H), 0.0f), ks.x);
    const float specular = (0.45f * spec) * 1.0f;
    const f3 base = frag_base01(f);
    float shadow = 1.0f;
    if (p.shadow) shadow = shadow_factor(p, wp, ndotl);
    // amb + direct: 0.18 * base + shadow * (diffuse * base + specular)
    f3 c = {0.18f * base.x + shadow * (diffuse * base.x + specular), 0.18f * base.y + shadow * (diffuse * base.y + specular),
            0.18f * base.z + shadow * (diffuse * base.z + specular)};
    f3 ibl_diffuse = {0.0f, 0.0f, 0.0f}, ibl_spec = {0.0f, 0.0f, 0.0f};
    if (p.ibl) {
        const f3 irr = ibl_sample_cube(p.ibl, 0, N);
        const float lod = ks.y * (float)(p.ibl_mips - 1);
        const f3 pre = ibl_sample_trilinear(p.ibl, p.ibl_mips, reflect3(f3{-V.x, -V.y, -V.z}, N), lod);
        // Math::schlick_fresnel(u.ibl_f0, max(0, N.V)) (shs_renderer.hpp:164-169)
        const float fx = 1.0f - saturate(g_max(0.0f, dot3(N, V)));
        const float fx2 = fx * fx;
        const float fx5 = fx2 * fx2 * fx;
        const float F = kn.z + (1.0f - kn.z) * fx5;
        const float kd = 1.0f - F;
        ibl_diffuse = {(kd * irr.x) * kn.x, (kd * irr.y) * kn.x, (kd * irr.z) * kn.x};
        ibl_spec = {((F * pre.x) * kn.y) * kn.w, ((F * pre.y) * kn.y) * kn.w, ((F * pre.z) * kn.y) * kn.w};
    }
    // result = ((amb + direct) + ibl_diffuse * baseColor) + ibl_spec
    const float pr = g_clamp01((c.x + ibl_diffuse.x * base.x) + ibl_spec.x) * 255;
    const float pg = g_clamp01((c.y + ibl_diffuse.y * base.y) + ibl_spec.y) * 255;
    const float pb = g_clamp01((c.z + ibl_diffuse.z * base.z) + ibl_spec.z) * 255;
    rgba = pack_rgba(pr, pg, pb);
    pq = make_float4(pr, pg, pb, shadow);
}

// ---- hello_water.cpp: the atmosphere shader, the water shader and the planar reflection ("water :line") ----

// fractf :759
__device__ __forceinline__ float fractf1(float x) { return x - floorf(x); }

// hash12 :771-777: q = fract2(p * vec2(123.34, 456.21)); q += dot(q, q + 34.345); fract(q.x * q.y).  Chaotic: every
// operation below is the reference's, in its order, and rounds once.
__device__ __forceinline__ float water_hash12(float px, float py) {
    float qx = fractf1(px * 123.34f), qy = fractf1(py * 456.21f);
    const float d = qx * (qx + 34.345f) + qy * (qy + 34.345f);
    qx = qx + d;
    qy = qy + d;
    return fractf1(qx * qy);
}

// noise2 :798-814 (i + vec2(0, 0) leaves every value hash12 can tell apart as it was)
__device__ __forceinline__ float water_noise2(float px, float py) {
    const float ix = floorf(px), iy = floorf(py);
    const float fx = px - ix, fy = py - iy;
    const float a = water_hash12(ix, iy);
    const float b = water_hash12(ix + 1.0f, iy);
    const float c = water_hash12(ix, iy + 1.0f);
    const float d = water_hash12(ix + 1.0f, iy + 1.0f);
    const float ux = (fx * fx) * (3.0f - 2.0f * fx), uy = (fy * fy) * (3.0f - 2.0f * fy);
    const float x1 = a + (b - a) * ux;
    const float x2 = c + (d - c) * ux;
    return x1 + (x2 - x1) * uy;
}

// fbm2 :816-826
__device__ __forceinline__ float water_fbm2(float px, float py) {
    float f = 0.0f, a = 0.5f;
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        f += a * water_noise2(px, py);
        px *= 2.02f;
        py *= 2.02f;
        a *= 0.5f;
    }
    return f;
}

// sampleN :902-917.  Its h0 and h1 are dead.  The four fbm2 arguments are (p +- vec2(e, 0)) * 1.2 and (p +- vec2(0, e)) * 1.2:
// a subtraction is the addition of the negated operand, signed zeros included, so one loop serves the four.
__device__ __forceinline__ f3 water_sample_n(float px, float py) {
    const float e = 0.18f;
    float hx = 0.0f, hz = 0.0f, prev = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const float ox = (k == 0) ? e : (k == 1) ? -e : (k == 2) ? 0.0f : -0.0f;
        const float oy = (k == 0) ? 0.0f : (k == 1) ? -0.0f : (k == 2) ? e : -e;
        const float f = water_fbm2((px + ox) * 1.2f, (py + oy) * 1.2f);
        if (k == 1) hx = prev - f;
        if (k == 3) hz = prev - f;
        prev = f;
    }
    return normalize3(f3{-hx * 2.4f, 1.0f, -hz * 2.4f});
}

// water_flow_normal_and_foam :862-930 after the host's part (RtWaterModel)
__device__ void water_normal_foam(const RtWaterModel &m, f3 wp, f3 &N, float &foam) {
    const float uvx = wp.x * m.perp[0] + wp.z * m.perp[1];
    const float uvy = (wp.x * m.fd[0] + wp.z * m.fd[1]) * 2.8f;
    const float bx = uvx * 0.055f, by = uvy * 0.055f;
    const f3 nA = water_sample_n((bx + m.j0[0]) + m.off0[0], (by + m.j0[1]) + m.off0[1]);
    const f3 nB = water_sample_n((bx + m.j1[0]) + m.off1[0], (by + m.j1[1]) + m.off1[1]);
    f3 n = normalize3(mix3(nA, nB, m.w));
    n = normalize3(f3{n.x + m.tilt[0], n.y + 0.0f, n.z + m.tilt[1]});
    N = n;
    const float curvature = sqrtf(n.x * n.x + n.z * n.z);
    foam = saturate((curvature - 0.55f) * 1.6f);
}

// (int)std::lround(x) for any x that is NaN or whose rounded value fits an int: halves away from zero on both sides
// of zero (lround_x86 covers [0, n - 1] only; the reflection lookup reaches -0.75 and n - 0.25)
__device__ __forceinline__ int lround_away_x86(float x) {
    if (!(x == x)) return 0;
    const float t = truncf(x);
    const float d = x - t;   // exact
    return (int)t + ((d >= 0.5f) ? 1 : ((d <= -0.5f) ? -1 : 0));
}

// shadow_uvz_from_world and shadow_factor_pcf_2x2 as hello_water.cpp has them (water :696-751).  Not the hard demo's
// lookup: a uv outside [0, 1] is lit before the PCF taps (the hard demo clamps the taps to the edge), and an empty
// texel (FLT_MAX) counts as lit whatever z is (the hard demo compares, which differs for a NaN z).
__device__ float shadow_factor_water(const RtParams &p, f3 wp, float ndotl) {
    float cx, cy, cz, cw;
    m4p(p.light_vp, wp.x, wp.y, wp.z, cx, cy, cz, cw);
    if (fabsf(cw) < 1e-6f) return 1.0f;
    const float nx = cx / cw, ny = cy / cw, z = cz / cw;
    if (z < 0.0f || z > 1.0f) return 1.0f;
    const float u = nx * 0.5f + 0.5f;
    const float v = 1.0f - (ny * 0.5f + 0.5f);
    const float slope = 1.0f - g_clamp01(ndotl);
    const float bias = p.bias_base + p.bias_slope * slope;
    if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) return 1.0f;
    if (!(p.flags & SHS_RT_PCF)) {
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
    const float d00 = sm_sample(p, x0, y0), d10 = sm_sample(p, x1, y0), d01 = sm_sample(p, x0, y1), d11 = sm_sample(p, x1, y1);
    const float s00 = (d00 == FLT_MAX) ? 1.0f : ((z <= d00 + bias) ? 1.0f : 0.0f);
    const float s10 = (d10 == FLT_MAX) ? 1.0f : ((z <= d10 + bias) ? 1.0f : 0.0f);
    const float s01 = (d01 == FLT_MAX) ? 1.0f : ((z <= d01 + bias) ? 1.0f : 0.0f);
    const float s11 = (d11 == FLT_MAX) ? 1.0f : ((z <= d11 + bias) ? 1.0f : 0.0f);
    return 0.25f * (((s00 + s10) + s01) + s11);
}

// pow(x, 5.0f), pow(x, 256.0f), pow(x, 520.0f): products in double rounded once, as pow64
__device__ __forceinline__ float pow5(float x) {
    const double d = (double)x, d2 = d * d;
    return (float)(d2 * d2 * d);
}
__device__ __forceinline__ float pow256(float x) {
    double d = (double)x;
#pragma unroll
    for (int i = 0; i < 8; ++i) d = d * d;
    return (float)d;
}
__device__ __forceinline__ float pow520(float x) {   // 512 and 8
    double d = (double)x;
    d = d * d; d = d * d; d = d * d;
    double e = d;
#pragma unroll
    for (int i = 0; i < 6; ++i) e = e * e;
    return (float)(e * d);
}

// One channel's way to the screen in hello_water.cpp (:984-992, :1088-1095): the exposure, tonemap_reinhard, gamma_2p2
// (glm::clamp, then pow), the channel * 255.  The byte is a rounding, clampi((int)lround(.), 0, 255), where the other
// shadings truncate: water_byte.
__device__ __forceinline__ float water_encode(float x) {
    x = x / (1.0f + x);
    x = powf(g_clamp01(x), 1.0f / 2.2f);
    return x * 255.0f;
}
__device__ __forceinline__ uint32_t water_byte(float x) { return (uint32_t)clampi(lround_away_x86(x), 0, 255); }

// The shown fragment of hello_water.cpp's camera pass (water :2060-2211, the hard demo's interpolation and velocity)
// through the shader its draw names: fragment_shader_full (:938-994, the atmosphere shader) or fragment_shader_water
// (:1000-1097).  One kernel holds both because one frame mixes them per pixel; the branch is per draw, so a wave
// diverges only where it straddles the water's silhouette.  What the two share is written once: V, the sky along the
// ray, the shadow lookup, the half vector, the fog and the way to the byte.
__device__ void shade_pixel_water(const RtParams &p, int32_t id, float u, float v, float w, uint32_t &rgba, float2 &vel, float4 &pq) {
    const Frag f(p, id, u, v, w);
    vel = frag_velocity(p, f.y, u, v, w);
    const f3 wp = f.world();
    const RtWaterGPU &wf = *p.water;
    const bool is_water = (reinterpret_cast<const uint32_t *>(p.water + 1)[f.r.draw] & SHS_RT_WATER_SURFACE) != 0u;
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 toc = sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp);
    const f3 V = normalize3(toc);
    // sky_color_simple(normalize(RAY), normalize(-L)) :157-170; its own normalize(sun_dir) is the host's (RtParams::sun)
    f3 sky;
    {
        const f3 ray = normalize3(f3{-V.x, -V.y, -V.z});
        const float t = saturate(ray.y * 0.5f + 0.5f);
        sky = mix3(f3{0.62f, 0.74f, 0.92f}, f3{0.10f, 0.22f, 0.55f}, t);
        const float sd = dot3(f3{wf.sun[0], wf.sun[1], wf.sun[2]}, normalize3(ray));
        const float sun = pow256(saturate(sd * 0.5f + 0.5f));
        sky = add3(sky, f3{(1.0f * sun) * 8.0f, (0.88f * sun) * 8.0f, (0.65f * sun) * 8.0f});
    }
    f3 N;
    float foam = 0.0f;
    if (is_water) water_normal_foam(wf.model, wp, N, foam);
    else N = f.normal();
    const float ndotl = dot3(N, L);
    float shadow = 1.0f;
    if (p.shadow) shadow = shadow_factor_water(p, wp, ndotl);
    const f3 H = normalize3(add3(L, V));
    const float ndoth = g_max(dot3(N, H), 0.0f);
    f3 hdr;
    float exposure;
    if (is_water) {
        const float NoV = g_clamp01(dot3(N, V));
        const float NoL = g_clamp01(ndotl);
        const float fresnel = 0.02f + (1.0f - 0.02f) * pow5(1.0f - NoV);
        f3 refl_col = sky;
        if (wf.refl) {   // the planar reflection :1021-1044
            float cx, cy, cz, cw;
            m4p(wf.refl_vp, wp.x, wp.y, wp.z, cx, cy, cz, cw);
            if (fabsf(cw) > 1e-6f) {
                const float rx_ndc = cx / cw, ry_ndc = cy / cw;
                if (rx_ndc >= -1.0f && rx_ndc <= 1.0f && ry_ndc >= -1.0f && ry_ndc <= 1.0f) {
                    float sx = (rx_ndc * 0.5f + 0.5f) * (float)(wf.refl_w - 1);
                    float sy = (1.0f - (ry_ndc * 0.5f + 0.5f)) * (float)(wf.refl_h - 1);
                    sx += N.x * 0.75f;
                    sy += N.z * 0.75f;
                    // sx lies in [-0.75, w - 0.25] or is NaN (|N.x| <= 1 or NaN): lround's halves away from zero on
                    // either side; a NaN gives (int)LONG_MIN = 0, so rx = 0 and ry_canvas = h - 1
                    const int rx = lround_away_x86(sx);
                    const int ry_screen = lround_away_x86(sy);
                    const int ry_canvas = (wf.refl_h - 1) - ry_screen;
                    // sample_canvas_nearest :146-151
                    refl_col = rgb01(wf.refl[(size_t)clampi(ry_canvas, 0, wf.refl_h - 1) * wf.refl_w + clampi(rx, 0, wf.refl_w - 1)]);
                }
            }
        }
        const float spec = pow520(ndoth);
        const float spec_kill = 1.0f - foam * 0.90f;
        const float specular = ((1.0f * spec) * 0.95f) * spec_kill;
        const float diffuse = (1.0f * NoL) * 0.05f;
        f3 surface = mix3(f3{0.03f, 0.12f, 0.16f}, refl_col, fresnel);
        const f3 foam_col = mix3(f3{0.75f, 0.85f, 0.95f}, sky, 0.25f);
        const float foam_gain = foam * (0.35f + 0.65f * (1.0f - NoV));
        surface = mix3(surface, foam_col, foam_gain);
        const float sd = shadow * diffuse, ss = shadow * specular;
        hdr = f3{surface.x * (sky.x * 0.12f + sd) + ss, surface.y * (sky.y * 0.12f + sd) + ss, surface.z * (sky.z * 0.12f + sd) + ss};
        exposure = 0.90f;
    } else {
        const f3 base = frag_base01(f);
        const float NoL = g_max(ndotl, 0.0f);
        const float diffuse = (1.0f * NoL) * 0.90f;
        const float specular = (1.0f * pow64(ndoth)) * 0.35f;
        const float lit = shadow * (diffuse + specular);
        hdr = f3{base.x * (sky.x * 0.08f + lit), base.y * (sky.y * 0.08f + lit), base.z * (sky.z * 0.08f + lit)};
        exposure = 1.00f;
    }
    // apply_fog_exp2 :172-176 over clampf(length(camera_pos - world_pos), 0, 250), then the exposure
    float dist = sqrtf(dot3(toc, toc));
    dist = (dist < 0.0f) ? 0.0f : (dist > 250.0f ? 250.0f : dist);
    const float tr = exp2f(-0.0065f * dist);
    const float fr = 1.0f - tr;
    const float pr = water_encode((hdr.x * tr + sky.x * fr) * exposure);
    const float pg = water_encode((hdr.y * tr + sky.y * fr) * exposure);
    const float pb = water_encode((hdr.z * tr + sky.z * fr) * exposure);
    rgba = water_byte(pr) | (water_byte(pg) << 8) | (water_byte(pb) << 16) | 0xff000000u;
    pq = make_float4(pr, pg, pb, shadow);
}

// ---- hello_multi_pass.cpp ("multi :line"; hello_camera_and_perobject_motion_blur.cpp carries the same text) and
// ---- hello_glowing_star.cpp ("star :line"): the shaders behind the unclipped raster -------------------------------

// The shown fragment of draw_triangle_tile_color_depth_motion (multi :575-595) / draw_triangle_color_depth_velocity_spec
// (star :407-431): screen-linear varyings, the velocity under the 0.0001 threshold, then blinn_phong_fragment_shader
// (multi :207-237; STAR false) or star_fragment_shader (star :269-308; STAR true), which also returns spec01.  The
// demos have no shadow map and no texture.  clampf (star :103-108) passes a NaN on: spec01 and the colour floats are NaN
// then, and the bytes 0.
// The same body serves the three plain demos (hello_per_object_motion_blur.cpp "per :line", hello_depth_of_field.cpp,
// hello_ping_pong.cpp), whose Blinn-Phong shader is multi :207-237 with another ambient term (per :145, dof :88,
// ping :72).  AMBIENT: ambientStrength, a type that carries the constant.  VELOCITY: how the velocity plane is filled,
// RT_VEL_CLAMPED (multi :583-591), RT_VEL_PER_PIXEL (velocity_fragment_shader, per :170-174) or RT_VEL_NONE (the plane
// stays zero: those demos have no velocity target).
struct RtAmbient35 { static constexpr float value = 0.35f; };
struct RtAmbient20 { static constexpr float value = 0.20f; };
struct RtAmbient15 { static constexpr float value = 0.15f; };
enum { RT_VEL_CLAMPED = 0, RT_VEL_PER_PIXEL = 1, RT_VEL_NONE = 2 };

template <bool STAR, class AMBIENT = RtAmbient35, int VELOCITY = RT_VEL_CLAMPED>
__device__ void shade_pixel_motion(const RtParams &p, int32_t id, float u, float v, float w, uint32_t &rgba, float2 &vel, float4 &pq,
                                   float &spec01) {
    const FragLinear f(p, id, u, v, w);
    if constexpr (VELOCITY == RT_VEL_CLAMPED) vel = frag_velocity(p, f.y, u, v, w, 0.0001f);
    else if constexpr (VELOCITY == RT_VEL_PER_PIXEL) vel = frag_velocity_ndc(p, f.y, u, v, w);
    const f3 wp = f.world();
    const f3 N = f.normal();
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    const float ambient = AMBIENT::value * 1.0f;
    const float diffuse = g_max(dot3(N, L), 0.0f) * 1.0f;
    const f3 H = normalize3(add3(L, V));
    const float ndoth = g_max(dot3(N, H), 0.0f);
    const f3 base = {f.dr.colf[0] / 255.0f, f.dr.colf[1] / 255.0f, f.dr.colf[2] / 255.0f};
    f3 result;
    if constexpr (STAR) {
        const float s = 3.85f * pow256(ndoth);
        spec01 = (s < 0.0f) ? 0.0f : (s > 1.0f ? 1.0f : s);
        const float lit = ambient + diffuse;
        // (ambient + diffuse) * (colour * 0.85) + spec01 * (1, 0.90, 0.55)
        result = {lit * (base.x * 0.85f) + spec01 * 1.0f, lit * (base.y * 0.85f) + spec01 * 0.90f, lit * (base.z * 0.85f) + spec01 * 0.55f};
    } else {
        const float specular = (0.5f * pow64(ndoth)) * 1.0f;
        const float lit = (ambient + diffuse) + specular;
        result = {lit * base.x, lit * base.y, lit * base.z};
    }
    const float pr = g_clamp01(result.x) * 255, pg = g_clamp01(result.y) * 255, pb = g_clamp01(result.z) * 255;
    rgba = pack_rgba(pr, pg, pb);
    pq = make_float4(pr, pg, pb, STAR ? spec01 : 1.0f);
}

}  // namespace
}  // namespace shs_dev
