// shs_canvas_rt_internal.hpp -- launch interface of shs_canvas_rt.hip: the Canvas render-target raster of
// hello-render-target/hello_shadow_mapping.cpp (shadow pass and shadowed camera pass; include/shs_gpu.h) and
// of hello_shadow_mapping_soft.cpp (the same passes with the PCSS fragment shader, shs_rt_frame::shading 1) and
// hello_pbr.cpp (the same passes with the GGX + IBL fragment shader, shading 2 through shs_rt_render_pbr) and
// hello_pbr_light_shafts.cpp (that shader under the PCSS factor, shading 3 through shs_rt_render_pbr_soft), and of the
// background pass behind any of them (skybox_background_pass over the legacy sky models, shs_rt_set_sky), and of
// hello_ibl_skybox.cpp (the hard demo's passes with the sky-lit fragment shader, shading 4 through
// shs_rt_render_skybox_ibl, which samples the bound sky per pixel), and of hello_water.cpp (the hard demo's passes with
// two fragment shaders chosen per draw, the atmosphere shader and the water shader over a planar reflection, shading 5
// through shs_rt_render_water), and of hello_multi_pass.cpp, hello_camera_and_perobject_motion_blur.cpp and
// hello_glowing_star.cpp (one raster without the near-plane clip, screen-linear varyings, back faces culled; shadings 6
// and 7 through shs_rt_render_motion, the latter with a fourth plane, spec01), and of hello_per_object_motion_blur.cpp,
// hello_depth_of_field.cpp and hello_ping_pong.cpp (that raster again with the depth plane in screen rows; shadings 8 to 10
// through shs_rt_render_plain), and of hello_ibl_skybox_optimized.cpp and hello_ibl_skybox_xsimd.cpp (the hard demo's
// camera raster with an IBL-lit Blinn-Phong shader of a per-draw exponent, shading 11 through shs_rt_render_ibl_phong, and
// the latter's edge-function shadow pass, shs_rt_render_shadow_edge).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace shs_dev {

// One sub-triangle as the raster walks it, 96 B (six float4s): the pixel-independent terms of
// Canvas::barycentric_coordinate over its screen corners {A, B, C}, the depth the pass tests at the corners
// (camera pass: view z; shadow pass: ndc z), the float bbox of the corners (NaN corners left out, as the
// reference's glm::min / glm::max fold leaves them out), the cull box and the corners' invw of the camera pass.
struct alignas(16) RtRec {
    float ax, ay, v0x, v0y;          // A, v0 = B - A
    float v1x, v1y, d00, d01;        // v1 = C - A
    float d11, denom, z0, z1;
    float z2;
    uint32_t flags;                  // RT_VALID | RT_NEG_AREA
    float minx, maxx;
    float miny, maxy;
    uint32_t gbx, gby;               // cull box, packed int16 (lo | hi << 16): outside it no pixel can pass
    float iw0, iw1, iw2;
    int32_t draw;
};
static_assert(sizeof(RtRec) == 96, "RtRec is staged as six float4s");
constexpr uint32_t RT_VALID = 1u, RT_NEG_AREA = 2u;

// The record of the edge-function shadow pass (hello_ibl_skybox_xsimd.cpp's ShadowTriProcessed :1016-1029 before the job's
// clamp) in an RtRec's slot, the same six float4s with `flags` where RtRec has it: the three edge functions E = A x + B y + C
// (:1071-1073), 1 / area, the corners' ndc z, (int)floor / (int)ceil of the corners' extent (:1040-1043 before std::max /
// std::min with the job) and that box clamped to the map, which every job's box lies in.
struct alignas(16) RtEdgeRec {
    float A0, B0, C0, A1;
    float B1, C1, A2, B2;
    float C2, inv_area, z0, z1;
    float z2;
    uint32_t flags;                  // RT_VALID
    int32_t fminx, cmaxx;            // (int)floor(min x), (int)ceil(max x)
    int32_t fminy, cmaxy;
    uint32_t gbx, gby;               // {fminx, cmaxx} / {fminy, cmaxy} clamped to the map, packed int16 (lo | hi << 16)
    uint32_t pad[3];
    int32_t draw;
};
static_assert(sizeof(RtEdgeRec) == sizeof(RtRec), "RtEdgeRec is staged in RtRec's six float4s");

// The corners' varyings (VaryingsFull) of a camera-pass sub-triangle, read by the pixels it shades.
struct alignas(16) RtVary {
    float pos[12];                   // position (clip), corner-major
    float prev[12];                  // prev_position
    float world[9];
    float nrm[9];
    float uv[6];
};
static_assert(sizeof(RtVary) == 192, "RtVary: 48 floats");

struct RtDrawGPU {
    const float *pos;                // soup: 9 floats per triangle
    const float *nrm;
    const float *uv;                 // 6 floats per triangle, or null
    const uint32_t *texels;          // or null: base colour
    int32_t tw, th;
    int32_t n_tris, base;            // the draw's first triangle in the submission
    float mvp[16], prev_mvp[16], model[16];
    float zm[16];                    // camera pass: view * model; shadow pass: light_vp * model
    float n3[12];                    // mat3(transpose(inverse(model))), column-major 3x3
    float colf[4];                   // (float)base_color.rgb
};

// The per-draw part of hello_pbr.cpp's Uniforms that fragment_shader_pbr reads (:474-482, :516-518), after the
// per-draw operations the host has done: 32 B, two dwordx4 loads of a shaded pixel.
struct alignas(16) RtPbrDrawGPU {
    float base[3];                   // srgb_to_linear(color_to_rgb01(baseColor_srgb)): three table entries
    float metallic;                  // saturate(mat.metallic)
    float roughness;                 // clampf(mat.roughness, min_roughness, 1)
    float ao;                        // saturate(mat.ao)
    float ibl_diffuse;               // saturate(ibl_diffuse_intensity)
    float ibl_specular;              // saturate(ibl_specular_intensity) * saturate(ibl_reflection_strength)
};
static_assert(sizeof(RtPbrDrawGPU) == 32, "RtPbrDrawGPU: two float4s");

// The per-draw knobs of hello_ibl_skybox.cpp's Uniforms (:336-339) after the three saturates of fragment_shader_full
// (:502, :509), which the host does; the products stay in the shader.  16 B: one dwordx4 load of a shaded pixel.
struct alignas(16) RtIblDrawGPU {
    float ambient;                   // saturate(ibl_ambient)
    float refl;                      // saturate(ibl_refl)
    float f0;                        // ibl_f0
    float refl_mix;                  // saturate(ibl_refl_mix)
};
static_assert(sizeof(RtIblDrawGPU) == 16, "RtIblDrawGPU: one float4");

// The per-draw knobs of hello_ibl_skybox_optimized.cpp's Uniforms (:757-764) after the three saturates of its
// fragment_shader_full (:943-944) and the lod's roughness (:929), which the host forms with the reference's own float
// operations; the products stay in the shader.  32 B: two dwordx4 loads of a shaded pixel.
struct alignas(16) RtIblPhongDrawGPU {
    float ambient;                   // saturate(ibl_ambient)
    float refl;                      // saturate(ibl_refl)
    float f0;                        // ibl_f0
    float refl_mix;                  // saturate(ibl_refl_mix)
    float shininess;                 // the exponent of the direct specular term
    float rough;                     // std::sqrt(2.0f / (shininess + 2.0f))
    float pad[2];
};
static_assert(sizeof(RtIblPhongDrawGPU) == 32, "RtIblPhongDrawGPU: two float4s");

// The EnvIBL levels (shs/resources/ibl.hpp:21-59) in one allocation of float4s: RT_IBL_LEVELS headers, then the
// texels, rgb padded to 16 B so that a bilinear corner is one dwordx4 load.  Header l holds, as int bits,
// {first texel, size}: level 0 is env_irradiance, level 1 + m is env_prefiltered_spec.mip[m].  Face f of a level
// starts size * size * f texels after its first; texel (x, y) of a face is at y * size + x.
constexpr int RT_IBL_LEVELS = 17;

// ---- skybox_background_pass (hello_pbr.cpp:733-799) over the legacy sky models of shs_renderer.hpp ----

constexpr int RT_SKY_NONE = 0, RT_SKY_ANALYTIC = 1, RT_SKY_CUBEMAP = 2;   // SHS_RT_SKY_*
constexpr int RT_SKY_REINHARD = 0, RT_SKY_CLAMP = 1;     // SHS_RT_SKY_ENCODE_*

// What AbstractSky::sample reads, after the operations the host has done once per shs_rt_set_sky.
struct RtSkyModel {
    // AnalyticSky (:552-611): everything that depends on the sun direction alone
    float s[3];                      // -normalize(sun_direction)
    float zenith[3], horizon[3];     // the two mixes over sun_height :574-575
    float ground[3];                 // ground_color :578-579
    float half_horizon[3];           // horizon_color * 0.5f :589
    float glow[3];                   // sun_glow_color :596
    // CubeMapSky (:432-517): the faces +X -X +Y -Y +Z -Z, the sRGB -> linear table and intensity_
    float intensity;
    const uint32_t *face[6];
    int32_t fw[6], fh[6];
    const float *srgb_lut;           // 256 floats: pow(c / 255, 2.2) with the host's libm
};

// ---- hello_water.cpp ("water :line"): what water_flow_normal_and_foam (:862-930) forms from the frame's time alone ----
// The host does these once per call with the reference's own float operations (shs_abi_canvas_rt.cpp water_model); the
// per-pixel ones stay in the shader.
struct RtWaterModel {
    float fd[2];                     // flow_dir = normalize(vec2(0.15, 1)) :877
    float perp[2];                   // flow_perp = (-fd.y, fd.x) :878
    float j0[2], j1[2];              // hash22(floor(time)) * 2, hash22(floor(time + 0.5)) * 2 :896-897
    float off0[2], off1[2];          // (flow_dir * (t0 - 0.5)) * 6, (flow_dir * (t1 - 0.5)) * 6 :899-900
    float w;                         // abs(t0 - 0.5) * 2 :891
    float tilt[2];                   // (fd.x, fd.y) * 0.15 :924 (the y component of the tilt is 0 * 0.15 = 0)
};

// The frame's part of hello_water.cpp's Uniforms that the two shaders of shading 5 read, in device memory behind the draw
// table (it changes every frame, as the table does); the n_draws flag words of shs_rt_water_draw follow it, element i
// going with draws[i].  Every read of it is wave-uniform.
struct alignas(16) RtWaterGPU {
    const uint32_t *refl;            // u.reflection_color: the context's reflection canvas in canvas rows, or null
    int32_t refl_w, refl_h;          // its own size, not the frame's
    float refl_vp[16];               // u.reflection_vp
    float sun[3];                    // normalize(normalize(-L)): sky_color_simple's sun_dir as it uses it (water :165)
    RtWaterModel model;
    uint32_t pad[3];
};
static_assert(sizeof(RtWaterGPU) % 16 == 0, "RtWaterGPU: the flag words follow it");

constexpr int RT_TW = 32, RT_TH = 8;     // raster tile: one 256-thread workgroup, one pixel per lane
constexpr int RT_CHUNK = 256;            // records examined (and at most staged in LDS) per round

struct RtParams {
    int32_t W, H, tile_w, tile_h;    // the target and the reference's tile job size
    int32_t n_draws, n_tris, n_recs;
    uint32_t clear_rgba, flags;      // SHS_RT_*
    float light_vp[16];
    float L[3];                      // normalize(-light_dir_world)
    float cam[3];
    float bias_base, bias_slope, max_velocity;
    const float *shadow;             // or null
    int32_t sw, sh;
    const RtDrawGPU *draws;
    RtRec *recs;
    RtVary *vary;
    unsigned long long *stats;       // 4 counters (shs_rt_stats), zeroed before the setup
    uint32_t *color;
    float *depth;                    // camera pass: view z in canvas rows; shadow pass: the map
    float2 *velocity;
    float4 *prequant;                // or null
    int32_t *ids;
    // shadings 1 and 3 only (appended: the hard instantiations' argument offsets stay as they were)
    const float4 *rot;               // per screen pixel py * W + px: {cos(ang), sin(ang), cos(ang2), sin(ang2)}
    float pcss_light, pcss_search, pcss_min, pcss_max, pcss_eps;   // shs_rt_pcss
    int32_t pcss_blockers, pcss_taps;
    int32_t simd_lanes;              // the edge-function shadow pass only: xsimd::batch<float>::size of the reference's build
    // shadings 2 and 3 only (appended likewise)
    const RtPbrDrawGPU *pbr_draws;   // element i goes with draws[i]
    const float *srgb_lut;           // 256 floats: pow(c / 255, 2.2) with the host's libm
    const float4 *ibl;               // the levels above, or null: u.ibl == nullptr
    int32_t ibl_mips;                // env_prefiltered_spec.mip_count()
    float pbr_exposure, pbr_intensity;   // shs_rt_pbr (min_roughness is folded into RtPbrDrawGPU::roughness)
    // shading 4 only (appended likewise)
    RtSkyModel sky;                  // u.sky: the sky of shs_rt_set_sky (read by the analytic / cubemap instantiations)
    // and shading 11, which reads ibl / ibl_mips above as shadings 2 and 3 do: one pointer's slot for the two tables, and
    // simd_lanes in the padding behind pcss_taps, because the struct's size is part of every kernel that takes it
    // (k_rt_setup<true> allocates two more registers when it grows)
    union {
        const RtIblDrawGPU *ibl_draws;              // shading 4: element i goes with draws[i]
        const RtIblPhongDrawGPU *ibl_phong_draws;   // shading 11: likewise
    };
    // shading 5 only (appended likewise): one pointer, the rest rides behind the draw table with the per-call upload
    const RtWaterGPU *water;
    // shading 7 only (appended likewise): RT_ColorDepthVelocitySpec::spec in canvas rows, 0 where no fragment is shown
    float *spec;
};
static_assert(sizeof(RtParams) == 512, "RtParams: new members go into its padding or share a slot (see ibl_draws)");

// sample_cubemap_linear_vec(env_irradiance, dir) and sample_prefiltered_spec_trilinear(spec, dir, lod) for a list
// of directions (shs_rt_ibl_samples): everything on the device
struct RtIblSamples {
    const float4 *ibl;
    int32_t ibl_mips, n;
    const float *dirs;               // 3 n
    const float *lod;                // n
    float *irr, *spec;               // 3 n each
};

// pcss_shadow_factor for a list of samples (shs_rt_pcss_samples): everything on the device
struct RtPcssSamples {
    const float *map;                // w x h, y down
    int32_t w, h, n;
    const float *uv;                 // 2 n
    const float *z, *bias;           // n each
    const float4 *rot;               // n: the rotations of each sample's screen pixel, formed by the host
    float *out;                      // n
    float pcss_light, pcss_search, pcss_min, pcss_max, pcss_eps;
    int32_t pcss_blockers, pcss_taps;
};

// The background pass's own parameters (not RtParams': the raster kernels' arguments stay as they were).
struct RtSkyParams {
    int32_t W, H;
    float aspect, tan_half_fov;      // float(W) / float(H); std::tan(glm::radians(fov) * 0.5f) with the host's libm
    float forward[3], right[3], up[3];   // normalised by the host
    float exposure;                  // SKY_EXPOSURE (the Reinhard encode only)
    const int32_t *ids;              // the raster's id plane: id < 0 shows sky
    uint32_t *color;
    float4 *prequant;                // or null
    RtSkyModel sky;
};

// sky.sample(dir) for a list of directions (shs_rt_sky_samples): everything on the device
struct RtSkySamples {
    int32_t n;
    const float *dirs;               // 3 n
    float *out;                      // 3 n
    RtSkyModel sky;
};

// water_flow_normal_and_foam for a list of points (shs_rt_water_samples): everything on the device
struct RtWaterSamples {
    int32_t n;
    const float *world;              // 3 n
    float *normal;                   // 3 n
    float *foam;                     // n
    RtWaterModel water;
};

}  // namespace shs_dev

namespace shs_internal {
// the background pass after a camera pass: one lane per pixel of the canvas rows (model, encode: SHS_RT_SKY_*)
hipError_t launch_canvas_rt_sky(const shs_dev::RtSkyParams &p, int model, int encode, hipStream_t s);
hipError_t launch_sky_samples(const shs_dev::RtSkySamples &q, int model, hipStream_t s);
// setup (one lane per input triangle) then raster (one workgroup per 32x8 tile) of either pass
// shading: shs_rt_frame::shading of the camera pass (0: fragment_shader_full, 1: fragment_shader_softshadow,
// 2: fragment_shader_pbr, 3: hello_pbr_light_shafts.cpp's fragment_shader_pbr, 4: hello_ibl_skybox.cpp's
// fragment_shader_full, 5: hello_water.cpp's fragment_shader_full / fragment_shader_water per draw, 6: hello_multi_pass.cpp's
// blinn_phong_fragment_shader, 7: hello_glowing_star.cpp's star_fragment_shader -- 6 and 7 behind the unclipped setup and
// the screen-linear raster of those demos, as are 8: hello_per_object_motion_blur.cpp's velocity_fragment_shader, 9:
// hello_depth_of_field.cpp's and 10: hello_ping_pong.cpp's blinn_phong_fragment_shader, whose depth plane is stored in
// screen rows); sky_model: u.sky of shading 4 (RT_SKY_*), which chooses among its three
// instantiations; 11: hello_ibl_skybox_optimized.cpp's / hello_ibl_skybox_xsimd.cpp's fragment_shader_full behind the clipped
// raster of shading 0.  edge_shadow (with shadow_pass): hello_ibl_skybox_xsimd.cpp's edge-function PASS0 (p.simd_lanes)
hipError_t launch_canvas_rt(const shs_dev::RtParams &p, bool shadow_pass, int shading, hipStream_t s, int sky_model = 0,
                            bool edge_shadow = false);
hipError_t launch_pcss_samples(const shs_dev::RtPcssSamples &q, hipStream_t s);
hipError_t launch_ibl_samples(const shs_dev::RtIblSamples &q, hipStream_t s);
hipError_t launch_water_samples(const shs_dev::RtWaterSamples &q, hipStream_t s);
}  // namespace shs_internal
