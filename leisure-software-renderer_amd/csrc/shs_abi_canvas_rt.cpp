// shs_abi_canvas_rt.cpp -- C ABI of the Canvas render-target raster (include/shs_gpu.h), paths relative to
// the reference's cpp-folders/src/hello-render-target/:
//   shs_rt_render_shadow  PASS0 of hello_shadow_mapping.cpp (:1320-1411 over draw_triangle_tile_shadow);
//   shs_rt_render         PASS1 (draw_triangle_tile_color_depth_motion_shadow :854-1022);
//   shs_ortho_lh_zo       ortho_lh_zo (:128-140);
// and of hello_shadow_mapping_soft.cpp: shs_rt_render with shading 1 (its PASS1, :845-1040), shs_rt_set_pcss (the
// constants :101-116), shs_rt_pcss_samples (pcss_shadow_factor :333-445 alone) and the per-pixel rotation table.
// and of hello_pbr.cpp ("pbr :line"): shs_rt_render_pbr (its PASS1, pbr :883-1045 with fragment_shader_pbr :627-727),
// shs_rt_set_pbr (the constants pbr :150-155), shs_rt_set_ibl (EnvIBL, shs/resources/ibl.hpp:21-59) and
// shs_rt_ibl_samples (the two IBL samplers alone, ibl.hpp:215-286);
// and of hello_pbr_light_shafts.cpp: shs_rt_render_pbr_soft (its PASS1, :1015-1180 with fragment_shader_pbr :768-850 over
// pcss_shadow_factor :650-762), which binds what shading 1 and shading 2 bind;
// and the background of hello_pbr.cpp, hello_pbr_light_shafts.cpp and hello_ibl_skybox.cpp: shs_rt_set_sky
// (skybox_background_pass pbr :733-799 over AnalyticSky / CubeMapSky, hello-shs-renderer/shs_renderer.hpp:432-611; the
// host does what depends on the sun direction and the camera alone) and shs_rt_sky_samples (sky.sample alone).
// and of hello_ibl_skybox.cpp ("ibl :line"): shs_rt_render_skybox_ibl (its PASS1, ibl :705-860 with fragment_shader_full
// :446-524), which hands the sky of shs_rt_set_sky to the raster's shade as well as to the background pass.
// and of hello_water.cpp ("water :line"): shs_rt_render_water (its PASS1A and PASS1B, water :1765-2211 with fragment_shader_full
// :938-994 and fragment_shader_water :1000-1097 per draw), shs_rt_keep_reflection / shs_rt_set_reflection (u.reflection_color)
// and shs_rt_water_samples (water_flow_normal_and_foam :862-930 alone); the host does what depends on the frame's time and
// the light direction alone (water_model).
// and of hello_multi_pass.cpp, hello_camera_and_perobject_motion_blur.cpp and hello_glowing_star.cpp: shs_rt_render_motion
// (their one unclipped raster, multi :525-599 / star :354-435, behind blinn_phong_fragment_shader multi :207-237 or
// star_fragment_shader star :269-308), shs_rt_resolve_spec / shs_rt_device_spec (RT_ColorDepthVelocitySpec::spec); their
// vertex shaders (multi :191-205, star :254-267) form the same two products and the same normal matrix.
// and of hello_per_object_motion_blur.cpp, hello_depth_of_field.cpp and hello_ping_pong.cpp: shs_rt_render_plain (that
// unclipped raster again, per_object :391-455 / dof :524-574 / ping_pong :352-400, shadings 8 to 10, with the depth plane in
// screen rows).
// and of hello_ibl_skybox_optimized.cpp ("opt :line") and hello_ibl_skybox_xsimd.cpp ("xsimd :line"): shs_rt_render_ibl_phong
// (their PASS1, opt :1125-1291 with fragment_shader_full opt :875-958, over the IBL of shs_rt_set_ibl) and
// shs_rt_render_shadow_edge (the xsimd demo's PASS0, draw_triangle_tile_shadow_xsimd xsimd :1016-1191).
// The host forms the matrix products the shaders form first -- u.view * u.model (vertex_shader_full :616),
// u.light_vp * u.model (shadow_vertex_shader :764) -- and the normal matrix with the GLM restatement in
// shs_glm.hpp.  Both passes are enqueued on the context stream; the shadow map, the planes and the records
// live in the context, so a camera pass reads the map of the shadow pass before it in stream order.
#include <cmath>
#include <cstddef>
#include <cstring>

#include "shs_canvas_rt_internal.hpp"
#include "shs_ctx.hpp"
#include "shs_glm.hpp"

namespace {

bool size_ok(shs_ctx *ctx, int W, int H, int tw, int th) {
    if (W > 0 && H > 0 && W <= 32767 && H <= 32767 && tw > 0 && th > 0) return true;
    ctx->err = "render target: 1 .. 32767 per side, reference tile size >= 1";
    return false;
}

// srgb_to_linear of a byte (shs_renderer.hpp:273-276 over color_to_rgb01 :291-293): pow(c / 255, 2.2) with the host's
// libm, as the reference evaluates it.  Both base-colour branches of fragment_shader_pbr start from bytes.
const float *srgb_table() {
    struct Lut {
        float v[256];
        Lut() {
            const volatile float gamma = 2.2f;   // (a run-time exponent: the libm call is not folded at compile time)
            for (int c = 0; c < 256; ++c) v[c] = std::pow(float(c) / 255.0f, gamma);
        }
    };
    static const Lut lut;
    return lut.v;
}

// The table on the device (shading 2's base colours, the cubemap sky's texels): uploaded once per context.
int ensure_srgb_table(shs_ctx *ctx) {
    if (ctx->rt_have_lut) return SHS_OK;
    if (ensure(ctx, ctx->rt_srgb_lut, 256)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->rt_srgb_lut.p, srgb_table(), 256 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->rt_have_lut = true;
    return SHS_OK;
}

float saturate(float v) { return (v < 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v); }
float clampf(float v, float lo, float hi) { return (v < lo) ? lo : (v > hi ? hi : v); }

// What a pass has beside its frame and its draws: one of the three at most (the shadow pass and shadings 0 and 1 have
// none), element i going with draws[i].  From it the pass builds its tail table, the bytes that ride behind the draw
// table in the same upload, and names the RtParams pointer that receives their device address.
struct PassExtras {
    const shs_rt_pbr_draw *pbr = nullptr;             // shadings 2 and 3: the per-draw uniforms
    const shs_rt_skybox_ibl_draw *ibl = nullptr;      // shading 4: the per-draw knobs
    const shs_rt_water_draw *water_draws = nullptr;   // shading 5: the per-draw flags
    const shs_rt_water *water = nullptr;              //   and the frame's uniforms
    const shs_rt_ibl_phong_draw *ibl_phong = nullptr; // shading 11: the per-draw knobs
    // the tail table: the context's rt_h_pbr, or `bytes` (a few draws long and alive for one call, so the context holds
    // no copy): the sky-lit pass's RtIblDrawGPUs, or the water pass's RtWaterGPU and the flag words behind it
    std::vector<unsigned char> bytes;
    const void *tail = nullptr;
    size_t tail_bytes = 0, tail_slot = 0;             // tail_slot: offsetof(RtParams, the pointer to the tail)
    void set_tail(const void *data, size_t n, size_t slot) { tail = data, tail_bytes = n, tail_slot = slot; }
    template <class T>
    void append(const T &v) { bytes.insert(bytes.end(), (const unsigned char *)&v, (const unsigned char *)(&v + 1)); }
};

// The draw table of either pass (zm: view for the camera pass, light_vp for the shadow pass) and the per-draw tail
// table of x.pbr or x.ibl.  Returns the triangle count, or -1 with ctx->err set.
int64_t build_draws(shs_ctx *ctx, const shs_rt_draw *draws, int32_t n, const float *zmat, bool camera, PassExtras &x) {
    ctx->rt_h_draws.clear();
    ctx->rt_h_pbr.clear();
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) {
        const shs_rt_draw &in = draws[i];
        if (in.mesh_id < 0 || in.mesh_id >= (int32_t)ctx->meshes.size() || !ctx->meshes[in.mesh_id].live ||
            ctx->meshes[in.mesh_id].lib) {
            ctx->err = "render-target draw: unknown soup mesh id";
            return -1;
        }
        const Mesh &m = ctx->meshes[in.mesh_id];
        shs_dev::RtDrawGPU o{};
        o.pos = m.pos;
        o.nrm = m.nrm;
        o.uv = m.soup_uv ? m.nrm + (size_t)m.n_tris * 9 : nullptr;
        if (camera && in.albedo_tex != 0) {
            if (in.albedo_tex < 0 || in.albedo_tex > (int32_t)ctx->textures.size() || !ctx->textures[(size_t)in.albedo_tex - 1].live) {
                ctx->err = "render-target draw: unknown texture id";
                return -1;
            }
            const Texture &t = ctx->textures[(size_t)in.albedo_tex - 1];
            o.texels = t.texels;
            o.tw = t.w;
            o.th = t.h;
        }
        o.n_tris = m.n_tris;
        o.base = (int32_t)total;
        std::memcpy(o.mvp, in.mvp, sizeof o.mvp);
        std::memcpy(o.prev_mvp, in.prev_mvp, sizeof o.prev_mvp);
        std::memcpy(o.model, in.model, sizeof o.model);
        shs_host::mul(zmat, in.model, o.zm);
        shs_host::normal_matrix(in.model, o.n3);
        for (int k = 0; k < 3; ++k) o.colf[k] = (float)in.base_color[k];
        if (x.pbr) {
            // u.normal_mat is the caller's (pbr :1482, :1557); the per-draw steps of fragment_shader_pbr (pbr :646-652,
            // :697, :706) are done here once
            const shs_rt_pbr_draw &m = x.pbr[i];
            std::memcpy(o.n3, m.normal_mat, 9 * sizeof(float));
            shs_dev::RtPbrDrawGPU g{};
            for (int k = 0; k < 3; ++k) g.base[k] = srgb_table()[in.base_color[k]];
            g.metallic = saturate(m.metallic);
            g.roughness = clampf(m.roughness, ctx->rt_pbr.min_roughness, 1.0f);
            g.ao = saturate(m.ao);
            g.ibl_diffuse = saturate(m.ibl_diffuse_intensity);
            g.ibl_specular = saturate(m.ibl_specular_intensity) * saturate(m.ibl_reflection_strength);
            ctx->rt_h_pbr.push_back(g);
        }
        if (x.ibl) {
            // the saturates of fragment_shader_full (ibl :502, :509), once per draw; their products stay in the shader
            const shs_rt_skybox_ibl_draw &k = x.ibl[i];
            x.append(shs_dev::RtIblDrawGPU{saturate(k.ibl_ambient), saturate(k.ibl_refl), k.ibl_f0, saturate(k.ibl_refl_mix)});
        }
        if (x.ibl_phong) {
            // the saturates of fragment_shader_full (opt :943-944) and the lod's roughness (opt :929), once per draw
            const shs_rt_ibl_phong_draw &k = x.ibl_phong[i];
            x.append(shs_dev::RtIblPhongDrawGPU{saturate(k.ibl_ambient), saturate(k.ibl_refl), k.ibl_f0, saturate(k.ibl_refl_mix), k.shininess,
                                                std::sqrt(2.0f / (k.shininess + 2.0f)), {0.0f, 0.0f}});
        }
        ctx->rt_h_draws.push_back(o);
        total += m.n_tris;
        if (total > (1 << 29)) {
            ctx->err = "render-target pass: more than 2^29 triangles";
            return -1;
        }
    }
    if (x.pbr) x.set_tail(ctx->rt_h_pbr.data(), ctx->rt_h_pbr.size() * sizeof(shs_dev::RtPbrDrawGPU), offsetof(shs_dev::RtParams, pbr_draws));
    if (x.ibl) x.set_tail(x.bytes.data(), x.bytes.size(), offsetof(shs_dev::RtParams, ibl_draws));
    if (x.ibl_phong) x.set_tail(x.bytes.data(), x.bytes.size(), offsetof(shs_dev::RtParams, ibl_phong_draws));
    return total;
}

// hash_u32 / hash01 (hello_shadow_mapping_soft.cpp:306-319) and the two rotations pcss_shadow_factor forms from
// the screen pixel (:359-360, :422): {cos(ang), sin(ang), cos(ang2), sin(ang2)} with the host libm, as rotate2
// (:320-325) takes them.  The kernels consume these; they never call a device sin / cos.
uint32_t hash_u32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
float hash01(uint32_t x) { return float(hash_u32(x) & 0x00FFFFFFu) / float(0x01000000u); }
void pixel_rotation(int px, int py, float out[4]) {
    const uint32_t seed = (uint32_t)px * 1973u ^ (uint32_t)py * 9277u ^ 0x9e3779b9u;
    const float ang = hash01(seed) * 6.2831853f;
    const float ang2 = hash01(seed ^ 0xB5297A4Du) * 6.2831853f;
    out[0] = std::cos(ang);
    out[1] = std::sin(ang);
    out[2] = std::cos(ang2);
    out[3] = std::sin(ang2);
}

// The rotation table of a W x H soft frame, entry py * W + px (screen rows): built and uploaded on the first
// soft frame of a size, kept until the size changes.  The upload is finished before the host copy goes.
int ensure_rotations(shs_ctx *ctx, int W, int H) {
    if (ctx->rt_rot.p && ctx->rt_rot_w == W && ctx->rt_rot_h == H) return SHS_OK;
    const size_t npx = (size_t)W * H;
    if (npx > ((size_t)1 << 26)) {
        ctx->err = "render-target frame: shadings 1 and 3 keep 16 B per pixel, at most 2^26 pixels";
        return SHS_ERR_INVALID;
    }
    ctx->rt_rot_w = ctx->rt_rot_h = 0;
    if (ensure(ctx, ctx->rt_rot, npx)) return SHS_ERR_HIP;
    std::vector<float> host(4 * npx);
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) pixel_rotation(px, py, &host[4 * ((size_t)py * W + px)]);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->rt_rot.p, host.data(), npx * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->rt_rot_w = W;
    ctx->rt_rot_h = H;
    return SHS_OK;
}

bool pcss_ok(const shs_rt_pcss &c) {
    return std::isfinite(c.light_uv_radius) && std::isfinite(c.search_radius_texels) && std::isfinite(c.min_filter_texels) &&
           std::isfinite(c.max_filter_texels) && std::isfinite(c.epsilon) && c.blocker_samples >= 0 && c.blocker_samples <= 64 &&
           c.pcf_samples >= 0 && c.pcf_samples <= 64;
}

// What water_flow_normal_and_foam (water :862-930) forms from the time alone, with its own float operations in its order
// (this file is compiled without contraction): fractf :759, hash22 :779-796, glm::normalize(vec2) = v * (1 / sqrt(dot)).
float fractf1(float x) { return x - std::floor(x); }
void water_hash22(float p, float out[2]) {
    float x = fractf1(p * 0.1031f);
    float y = fractf1(p * 0.1030f);
    float z = fractf1(p * 0.0973f);
    const float d = x * (y + 19.19f) + y * (z + 19.19f) + z * (x + 19.19f);
    x = fractf1(x + d);
    y = fractf1(y + d);
    z = fractf1(z + d);
    out[0] = fractf1((x + y) * z);
    out[1] = fractf1((x + z) * y);
}
shs_dev::RtWaterModel water_model(float time_sec) {
    shs_dev::RtWaterModel m{};
    const float vx = 0.15f, vy = 1.0f;
    const float inv = 1.0f / std::sqrt(vx * vx + vy * vy);
    m.fd[0] = vx * inv;
    m.fd[1] = vy * inv;
    m.perp[0] = -m.fd[1];
    m.perp[1] = m.fd[0];
    const float time = time_sec * 0.18f;
    const float t0 = fractf1(time);
    const float t1 = fractf1(time + 0.5f);
    m.w = std::fabs(t0 - 0.5f) * 2.0f;
    float h[2];
    water_hash22(std::floor(time), h);
    m.j0[0] = h[0] * 2.0f; m.j0[1] = h[1] * 2.0f;
    water_hash22(std::floor(time + 0.5f), h);
    m.j1[0] = h[0] * 2.0f; m.j1[1] = h[1] * 2.0f;
    for (int k = 0; k < 2; ++k) {
        m.off0[k] = (m.fd[k] * (t0 - 0.5f)) * 6.0f;
        m.off1[k] = (m.fd[k] * (t1 - 0.5f)) * 6.0f;
        m.tilt[k] = m.fd[k] * 0.15f;
    }
    return m;
}

// The seven constants of shs_rt_pcss into the kernel arguments that carry them (RtParams, RtPcssSamples)
template <class Args>
void fill_pcss(Args &a, const shs_rt_pcss &c) {
    a.pcss_light = c.light_uv_radius;
    a.pcss_search = c.search_radius_texels;
    a.pcss_min = c.min_filter_texels;
    a.pcss_max = c.max_filter_texels;
    a.pcss_eps = c.epsilon;
    a.pcss_blockers = c.blocker_samples;
    a.pcss_taps = c.pcf_samples;
}

int upload_and_launch(shs_ctx *ctx, shs_dev::RtParams &p, bool shadow_pass, int shading, int sky_model, const PassExtras &x,
                      bool edge_shadow = false) {
    const size_t nd = ctx->rt_h_draws.size();
    // the pass's tail table rides behind the draw table (sizeof(RtDrawGPU) is a multiple of 16): one copy
    static_assert(sizeof(shs_dev::RtDrawGPU) % 16 == 0, "the material table behind the draws is read as float4s");
    const size_t tail = x.tail_bytes;
    const size_t extra = (tail + sizeof(shs_dev::RtDrawGPU) - 1) / sizeof(shs_dev::RtDrawGPU);
    const size_t nslot = nd + extra;
    if (ensure(ctx, ctx->rt_draws, std::max<size_t>(nslot, 1)) || ensure(ctx, ctx->rt_recs, std::max<size_t>((size_t)p.n_recs, 1)) ||
        ensure(ctx, ctx->rt_stats, 4))
        return SHS_ERR_HIP;
    if (!shadow_pass && ensure(ctx, ctx->rt_vary, std::max<size_t>((size_t)p.n_recs, 1))) return SHS_ERR_HIP;
    if (nd || tail) {   // (the water pass has a tail without a draw)
        const int k = (int)(ctx->rt_pin_next++ & 1u);
        if (!ctx->rt_pin_ev[k]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->rt_pin_ev[k], hipEventDisableTiming));
        else HIP_TRY(ctx, hipEventSynchronize(ctx->rt_pin_ev[k]));
        if (ctx->rt_pin_cap[k] < nslot) {
            if (ctx->rt_pin[k]) HIP_TRY(ctx, hipHostFree(ctx->rt_pin[k]));
            ctx->rt_pin[k] = nullptr;
            ctx->rt_pin_cap[k] = 0;
            HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->rt_pin[k]), nslot * sizeof(shs_dev::RtDrawGPU), hipHostMallocDefault));
            ctx->rt_pin_cap[k] = nslot;
        }
        std::memcpy(ctx->rt_pin[k], ctx->rt_h_draws.data(), nd * sizeof(shs_dev::RtDrawGPU));
        if (tail) std::memcpy(ctx->rt_pin[k] + nd, x.tail, tail);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->rt_draws.p, ctx->rt_pin[k], nd * sizeof(shs_dev::RtDrawGPU) + tail, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->rt_pin_ev[k], ctx->stream));
    }
    if (!shadow_pass) HIP_TRY(ctx, hipMemsetAsync(ctx->rt_stats.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
    p.draws = ctx->rt_draws.p;
    if (tail) {   // pbr_draws, ibl_draws or water; the other two stay null
        const void *dev = ctx->rt_draws.p + nd;
        std::memcpy(reinterpret_cast<char *>(&p) + x.tail_slot, &dev, sizeof dev);
    }
    p.recs = ctx->rt_recs.p;
    p.vary = ctx->rt_vary.p;
    p.stats = ctx->rt_stats.p;
    HIP_TRY(ctx, shs_internal::launch_canvas_rt(p, shadow_pass, shading, ctx->stream, sky_model, edge_shadow));
    return SHS_OK;
}

// PASS1 of the six demos: x empty for shading 0 / 1 (shs_rt_render), x.pbr for shading 2 (shs_rt_render_pbr) and 3
// (shs_rt_render_pbr_soft), x.ibl for shading 4 (shs_rt_render_skybox_ibl), x.water_draws and x.water for shading 5
// (shs_rt_render_water); and the one camera pass of the three unclipped demos, x empty, for shadings 6 and 7
// (shs_rt_render_motion) and 8 to 10 (shs_rt_render_plain); and PASS1 of the two later IBL demos, x.ibl_phong for shading 11
// (shs_rt_render_ibl_phong).  Nothing of the context changes before the last rejection.
int render_camera(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, int32_t n_draws, PassExtras x) {
    if (!size_ok(ctx, f->width, f->height, f->ref_tile_w, f->ref_tile_h)) return SHS_ERR_INVALID;
    if (f->flags & ~(SHS_RT_USE_SHADOW | SHS_RT_PCF | SHS_RT_PREQUANT)) {
        ctx->err = "render-target frame: unknown flags";
        return SHS_ERR_INVALID;
    }
    if ((f->flags & SHS_RT_USE_SHADOW) && !ctx->rt_have_shadow) {
        ctx->err = "render-target frame: SHS_RT_USE_SHADOW without a shs_rt_render_shadow before it";
        return SHS_ERR_INVALID;
    }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const int64_t n_tris = build_draws(ctx, draws, n_draws, f->view, true, x);
    if (n_tris < 0) return SHS_ERR_INVALID;
    const size_t npx = (size_t)f->width * f->height;
    const bool pq = (f->flags & SHS_RT_PREQUANT) != 0;
    if (ensure(ctx, ctx->rt_color, npx) || ensure(ctx, ctx->rt_depth, npx) || ensure(ctx, ctx->rt_vel, 2 * npx) ||
        ensure(ctx, ctx->rt_ids, npx) || (pq && ensure(ctx, ctx->rt_pq, npx)) || (f->shading == 7 && ensure(ctx, ctx->rt_spec, npx)))
        return SHS_ERR_HIP;
    shs_dev::RtParams p{};
    p.W = f->width; p.H = f->height;
    p.tile_w = std::min(f->ref_tile_w, f->width);   // (a job larger than the target is the whole target)
    p.tile_h = std::min(f->ref_tile_h, f->height);
    p.n_draws = n_draws;
    p.n_tris = (int32_t)n_tris;
    p.n_recs = 2 * (int32_t)n_tris;
    std::memcpy(&p.clear_rgba, f->clear_color, 4);
    p.flags = f->flags;
    std::memcpy(p.light_vp, f->light_vp, sizeof p.light_vp);
    // glm::normalize(-u.light_dir_world) (:702), the same for every fragment
    const shs_host::vec3 L = shs_host::gnormalize(shs_host::gneg({f->light_dir_world[0], f->light_dir_world[1], f->light_dir_world[2]}));
    p.L[0] = L.x; p.L[1] = L.y; p.L[2] = L.z;
    std::memcpy(p.cam, f->camera_pos, sizeof p.cam);
    p.bias_base = f->bias_base;
    p.bias_slope = f->bias_slope;
    p.max_velocity = f->max_velocity_px;
    if (f->flags & SHS_RT_USE_SHADOW) {
        p.shadow = ctx->rt_shadow.p;
        p.sw = ctx->rt_sw;
        p.sh = ctx->rt_sh;
    }
    p.color = ctx->rt_color.p;
    p.depth = ctx->rt_depth.p;
    p.velocity = reinterpret_cast<float2 *>(ctx->rt_vel.p);
    p.prequant = pq ? ctx->rt_pq.p : nullptr;
    p.ids = ctx->rt_ids.p;
    p.spec = f->shading == 7 ? ctx->rt_spec.p : nullptr;
    if (f->shading == 1 || f->shading == 3) {
        const int rr = ensure_rotations(ctx, f->width, f->height);
        if (rr) return rr;
        p.rot = ctx->rt_rot.p;
        fill_pcss(p, ctx->rt_pcss);
    }
    if (f->shading == 11) {   // u.ibl: the levels of shs_rt_set_ibl, as shadings 2 and 3 read them
        p.ibl = ctx->rt_ibl_mips > 0 ? ctx->rt_ibl.p : nullptr;
        p.ibl_mips = ctx->rt_ibl_mips;
    }
    if (f->shading == 2 || f->shading == 3) {
        if (ensure_srgb_table(ctx)) return SHS_ERR_HIP;
        p.srgb_lut = ctx->rt_srgb_lut.p;
        p.ibl = ctx->rt_ibl_mips > 0 ? ctx->rt_ibl.p : nullptr;
        p.ibl_mips = ctx->rt_ibl_mips;
        p.pbr_exposure = ctx->rt_pbr.exposure;
        p.pbr_intensity = ctx->rt_pbr.direct_intensity;
    }
    int sky_model = SHS_RT_SKY_NONE;
    if (f->shading == 4) {
        // u.sky (ibl :1298): the sky the background pass below draws, as shs_rt_set_sky converted it
        sky_model = ctx->rt_sky.model;
        p.sky = ctx->rt_sky_model;
    }
    if (f->shading == 5) {
        shs_dev::RtWaterGPU g{};
        if (x.water->flags & SHS_RT_WATER_REFLECTION) {
            g.refl = ctx->rt_refl.p;
            g.refl_w = ctx->rt_refl_w;
            g.refl_h = ctx->rt_refl_h;
        }
        std::memcpy(g.refl_vp, x.water->reflection_vp, sizeof g.refl_vp);
        // sky_color_simple(.., glm::normalize(-L)) normalises its sun_dir again (water :967, :165)
        const shs_host::vec3 sun = shs_host::gnormalize(shs_host::gnormalize(shs_host::gneg(L)));
        g.sun[0] = sun.x; g.sun[1] = sun.y; g.sun[2] = sun.z;
        g.model = water_model(x.water->time_sec);
        x.append(g);
        for (int32_t i = 0; i < n_draws; ++i) x.append(x.water_draws[i].flags);
        x.set_tail(x.bytes.data(), x.bytes.size(), offsetof(shs_dev::RtParams, water));
    }
    int rc = upload_and_launch(ctx, p, false, f->shading, sky_model, x);
    if (!rc && ctx->rt_sky.model != SHS_RT_SKY_NONE) {
        // skybox_background_pass (pbr :733-799) behind the triangles: the pixels the raster left without a fragment
        shs_dev::RtSkyParams q{};
        q.W = f->width; q.H = f->height;
        q.aspect = float(f->width) / float(f->height);
        q.tan_half_fov = ctx->rt_sky_tan;
        std::memcpy(q.forward, ctx->rt_sky_cam, sizeof q.forward);
        std::memcpy(q.right, ctx->rt_sky_cam + 3, sizeof q.right);
        std::memcpy(q.up, ctx->rt_sky_cam + 6, sizeof q.up);
        q.exposure = ctx->rt_sky.exposure;
        q.ids = p.ids;
        q.color = p.color;
        q.prequant = p.prequant;
        q.sky = ctx->rt_sky_model;
        const hipError_t e = shs_internal::launch_canvas_rt_sky(q, ctx->rt_sky.model, ctx->rt_sky.encode, ctx->stream);
        if (e != hipSuccess) {
            ctx->err = hipGetErrorString(e);
            rc = SHS_ERR_HIP;
        }
    }
    if (rc) {
        ctx->rt_have_frame = false;
        return rc;
    }
    ctx->rt_w = f->width;
    ctx->rt_h = f->height;
    ctx->rt_n_tris = n_tris;
    ctx->rt_have_frame = true;
    ctx->rt_have_pq = pq;
    ctx->rt_have_spec = f->shading == 7;
    return SHS_OK;
}

// shs_rt_render_pbr and shs_rt_render_pbr_soft: the same entry but for the shading it takes and how it names itself
int render_pbr(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, const shs_rt_pbr_draw *pbr_draws, int32_t n_draws,
               int32_t shading, const char *entry, const char *shader) {
    if (!ctx || !f || n_draws < 0 || (n_draws > 0 && (!draws || !pbr_draws))) return SHS_ERR_INVALID;
    if (f->shading != shading) {
        ctx->err = std::string(entry) + ": shading " + std::to_string(f->shading) + " (" + std::to_string(shading) + ": " + shader + ")";
        return SHS_ERR_INVALID;
    }
    static const shs_rt_pbr_draw none{};
    return render_camera(ctx, f, draws, n_draws, PassExtras{n_draws > 0 ? pbr_draws : &none});
}

}  // namespace

extern "C" {

// PASS0 into the context's shadow map.  simd_lanes 0: draw_triangle_tile_shadow (shs_rt_render_shadow); else
// hello_ibl_skybox_xsimd.cpp's draw_triangle_tile_shadow_xsimd with that batch size (shs_rt_render_shadow_edge).
static int render_shadow(shs_ctx *ctx, int32_t w, int32_t h, int32_t ref_tile_w, int32_t ref_tile_h, const float light_vp[16],
                         const shs_rt_draw *casters, int32_t n_casters, int32_t simd_lanes) {
    if (!ctx || !light_vp || n_casters < 0 || (n_casters > 0 && !casters)) return SHS_ERR_INVALID;
    if (!size_ok(ctx, w, h, ref_tile_w, ref_tile_h)) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    PassExtras none;
    const int64_t n_tris = build_draws(ctx, casters, n_casters, light_vp, false, none);
    if (n_tris < 0) return SHS_ERR_INVALID;
    if (ensure(ctx, ctx->rt_shadow, (size_t)w * h)) return SHS_ERR_HIP;
    shs_dev::RtParams p{};
    p.W = w; p.H = h;
    p.tile_w = std::min(ref_tile_w, w);   // (a job larger than the target is the whole target)
    p.tile_h = std::min(ref_tile_h, h);
    p.n_draws = n_casters;
    p.n_tris = (int32_t)n_tris;
    p.n_recs = (int32_t)n_tris;
    p.depth = ctx->rt_shadow.p;
    p.simd_lanes = simd_lanes;
    // the shadow pass shares the stats words with the camera pass: its own count is not reported
    const int rc = upload_and_launch(ctx, p, true, 0, SHS_RT_SKY_NONE, none, simd_lanes != 0);
    if (rc) return rc;
    ctx->rt_sw = w;
    ctx->rt_sh = h;
    ctx->rt_have_shadow = true;
    return SHS_OK;
}

int shs_rt_render_shadow(shs_ctx *ctx, int32_t w, int32_t h, int32_t ref_tile_w, int32_t ref_tile_h, const float light_vp[16],
                         const shs_rt_draw *casters, int32_t n_casters) {
    return render_shadow(ctx, w, h, ref_tile_w, ref_tile_h, light_vp, casters, n_casters, 0);
}

int shs_rt_render_shadow_edge(shs_ctx *ctx, int32_t w, int32_t h, int32_t ref_tile_w, int32_t ref_tile_h, const float light_vp[16],
                              const shs_rt_draw *casters, int32_t n_casters, int32_t simd_lanes) {
    if (!ctx) return SHS_ERR_INVALID;
    if (simd_lanes != 1 && simd_lanes != 2 && simd_lanes != 4 && simd_lanes != 8 && simd_lanes != 16) {
        ctx->err = "shs_rt_render_shadow_edge: simd_lanes " + std::to_string(simd_lanes) + " (xsimd::batch<float>::size: 1, 2, 4, 8 or 16)";
        return SHS_ERR_INVALID;
    }
    return render_shadow(ctx, w, h, ref_tile_w, ref_tile_h, light_vp, casters, n_casters, simd_lanes);
}

int shs_rt_render_ibl_phong(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, const shs_rt_ibl_phong_draw *ibl_draws,
                            int32_t n_draws) {
    if (!ctx || !f || n_draws < 0 || (n_draws > 0 && (!draws || !ibl_draws))) return SHS_ERR_INVALID;
    if (f->shading != 11) {
        ctx->err = "shs_rt_render_ibl_phong: shading " + std::to_string(f->shading) +
                   " (11: hello_ibl_skybox_optimized.cpp's and hello_ibl_skybox_xsimd.cpp's fragment_shader_full)";
        return SHS_ERR_INVALID;
    }
    for (int32_t i = 0; i < n_draws; ++i) {
        const shs_rt_ibl_phong_draw &k = ibl_draws[i];
        if (!(std::isfinite(k.ibl_ambient) && std::isfinite(k.ibl_refl) && std::isfinite(k.ibl_f0) && std::isfinite(k.ibl_refl_mix) &&
              std::isfinite(k.shininess))) {
            ctx->err = "shs_rt_render_ibl_phong: a non-finite knob";
            return SHS_ERR_INVALID;
        }
        if (k.shininess < 0.0f) {
            ctx->err = "shs_rt_render_ibl_phong: shininess < 0";
            return SHS_ERR_INVALID;
        }
    }
    static const shs_rt_ibl_phong_draw none{};
    PassExtras x;
    x.ibl_phong = n_draws > 0 ? ibl_draws : &none;
    return render_camera(ctx, f, draws, n_draws, std::move(x));
}

int shs_rt_render(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, int32_t n_draws) {
    if (!ctx || !f || n_draws < 0 || (n_draws > 0 && !draws)) return SHS_ERR_INVALID;
    if (f->shading != 0 && f->shading != 1) {
        ctx->err = "render-target frame: shading " + std::to_string(f->shading) +
                   " (0: fragment_shader_full, 1: fragment_shader_softshadow; 2, fragment_shader_pbr, goes through shs_rt_render_pbr; 11, the later IBL demos' fragment_shader_full, through shs_rt_render_ibl_phong)";
        return SHS_ERR_INVALID;
    }
    return render_camera(ctx, f, draws, n_draws, PassExtras{});
}

int shs_rt_render_pbr(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, const shs_rt_pbr_draw *pbr_draws, int32_t n_draws) {
    return render_pbr(ctx, f, draws, pbr_draws, n_draws, 2, "shs_rt_render_pbr", "fragment_shader_pbr");
}

int shs_rt_render_pbr_soft(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, const shs_rt_pbr_draw *pbr_draws, int32_t n_draws) {
    return render_pbr(ctx, f, draws, pbr_draws, n_draws, 3, "shs_rt_render_pbr_soft", "fragment_shader_pbr under PCSS");
}

int shs_rt_render_skybox_ibl(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, const shs_rt_skybox_ibl_draw *ibl_draws,
                             int32_t n_draws) {
    if (!ctx || !f || n_draws < 0 || (n_draws > 0 && (!draws || !ibl_draws))) return SHS_ERR_INVALID;
    if (f->shading != 4) {
        ctx->err = "shs_rt_render_skybox_ibl: shading " + std::to_string(f->shading) + " (4: hello_ibl_skybox.cpp's fragment_shader_full)";
        return SHS_ERR_INVALID;
    }
    for (int32_t i = 0; i < n_draws; ++i) {
        const shs_rt_skybox_ibl_draw &k = ibl_draws[i];
        if (!(std::isfinite(k.ibl_ambient) && std::isfinite(k.ibl_refl) && std::isfinite(k.ibl_f0) && std::isfinite(k.ibl_refl_mix))) {
            ctx->err = "shs_rt_render_skybox_ibl: a non-finite knob";
            return SHS_ERR_INVALID;
        }
    }
    static const shs_rt_skybox_ibl_draw none{};
    return render_camera(ctx, f, draws, n_draws, PassExtras{nullptr, n_draws > 0 ? ibl_draws : &none});
}

int shs_rt_render_water(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, const shs_rt_water_draw *water_draws,
                        const shs_rt_water *water, int32_t n_draws) {
    if (!ctx || !f || !water || n_draws < 0 || (n_draws > 0 && (!draws || !water_draws))) return SHS_ERR_INVALID;
    if (f->shading != 5) {
        ctx->err = "shs_rt_render_water: shading " + std::to_string(f->shading) + " (5: hello_water.cpp's two fragment shaders)";
        return SHS_ERR_INVALID;
    }
    for (int32_t i = 0; i < n_draws; ++i) {
        if (water_draws[i].flags & ~SHS_RT_WATER_SURFACE) {
            ctx->err = "shs_rt_render_water: unknown shs_rt_water_draw flags";
            return SHS_ERR_INVALID;
        }
    }
    if (water->flags & ~SHS_RT_WATER_REFLECTION) {
        ctx->err = "shs_rt_render_water: unknown shs_rt_water flags";
        return SHS_ERR_INVALID;
    }
    if ((water->flags & SHS_RT_WATER_REFLECTION) && !ctx->rt_have_refl) {
        ctx->err = "shs_rt_render_water: SHS_RT_WATER_REFLECTION without a reflection canvas (shs_rt_keep_reflection, shs_rt_set_reflection)";
        return SHS_ERR_INVALID;
    }
    if (!std::isfinite(water->time_sec)) {
        ctx->err = "shs_rt_render_water: a non-finite time_sec";
        return SHS_ERR_INVALID;
    }
    return render_camera(ctx, f, draws, n_draws, PassExtras{nullptr, nullptr, water_draws, water});
}

int shs_rt_render_motion(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, int32_t n_draws) {
    if (!ctx || !f || n_draws < 0 || (n_draws > 0 && !draws)) return SHS_ERR_INVALID;
    if (f->shading != 6 && f->shading != 7) {
        ctx->err = "shs_rt_render_motion: shading " + std::to_string(f->shading) +
                   " (6: hello_multi_pass.cpp's blinn_phong_fragment_shader, 7: hello_glowing_star.cpp's star_fragment_shader)";
        return SHS_ERR_INVALID;
    }
    if (f->flags & (SHS_RT_USE_SHADOW | SHS_RT_PCF)) {
        ctx->err = "shs_rt_render_motion: SHS_RT_USE_SHADOW / SHS_RT_PCF (these demos have no shadow map)";
        return SHS_ERR_INVALID;
    }
    if (!(std::isfinite(f->max_velocity_px) && f->max_velocity_px >= 0.0f)) {
        ctx->err = "shs_rt_render_motion: max_velocity_px is not finite or is negative";
        return SHS_ERR_INVALID;
    }
    for (int32_t i = 0; i < n_draws; ++i) {
        if (draws[i].albedo_tex != 0) {   // (the shaders read u.color only)
            ctx->err = "shs_rt_render_motion: a draw with albedo_tex (shadings 6 and 7 have no texture)";
            return SHS_ERR_INVALID;
        }
    }
    return render_camera(ctx, f, draws, n_draws, PassExtras{});
}

int shs_rt_render_plain(shs_ctx *ctx, const shs_rt_frame *f, const shs_rt_draw *draws, int32_t n_draws) {
    if (!ctx || !f || n_draws < 0 || (n_draws > 0 && !draws)) return SHS_ERR_INVALID;
    if (f->shading < 8 || f->shading > 10) {
        ctx->err = "shs_rt_render_plain: shading " + std::to_string(f->shading) +
                   " (8: hello_per_object_motion_blur.cpp's velocity_fragment_shader, 9: hello_depth_of_field.cpp's and 10: "
                   "hello_ping_pong.cpp's blinn_phong_fragment_shader)";
        return SHS_ERR_INVALID;
    }
    if (f->flags & (SHS_RT_USE_SHADOW | SHS_RT_PCF)) {
        ctx->err = "shs_rt_render_plain: SHS_RT_USE_SHADOW / SHS_RT_PCF (these demos have no shadow map)";
        return SHS_ERR_INVALID;
    }
    for (int32_t i = 0; i < n_draws; ++i) {
        if (draws[i].albedo_tex != 0) {   // (the shaders read u.color only)
            ctx->err = "shs_rt_render_plain: a draw with albedo_tex (shadings 8 to 10 have no texture)";
            return SHS_ERR_INVALID;
        }
    }
    // (shading 10: ping :50-59 forms no view z; the view * model product the draw table carries goes unread on the device)
    return render_camera(ctx, f, draws, n_draws, PassExtras{});
}

int shs_rt_resolve_spec(shs_ctx *ctx, float *spec) {
    if (!ctx || !spec || !ctx->rt_have_frame || !ctx->rt_have_spec) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(spec, ctx->rt_spec.p, (size_t)ctx->rt_w * ctx->rt_h * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SHS_OK;
}

int shs_rt_device_spec(shs_ctx *ctx, void **spec_dev) {
    if (!ctx || !ctx->rt_have_frame || !ctx->rt_have_spec) return SHS_ERR_INVALID;
    if (spec_dev) *spec_dev = ctx->rt_spec.p;
    return SHS_OK;
}

int shs_rt_keep_reflection(shs_ctx *ctx) {
    if (!ctx) return SHS_ERR_INVALID;
    if (!ctx->rt_have_frame) {
        ctx->err = "shs_rt_keep_reflection: no camera pass before it";
        return SHS_ERR_INVALID;
    }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t npx = (size_t)ctx->rt_w * ctx->rt_h;
    ctx->rt_have_refl = false;
    if (ensure(ctx, ctx->rt_refl, npx)) return SHS_ERR_HIP;
    // in stream order after the camera pass (and its background pass) and before whatever reads the canvas
    HIP_TRY(ctx, hipMemcpyAsync(ctx->rt_refl.p, ctx->rt_color.p, npx * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    ctx->rt_refl_w = ctx->rt_w;
    ctx->rt_refl_h = ctx->rt_h;
    ctx->rt_have_refl = true;
    return SHS_OK;
}

int shs_rt_set_reflection(shs_ctx *ctx, const uint8_t *rgba, int32_t w, int32_t h) {
    if (!ctx) return SHS_ERR_INVALID;
    if (!rgba) {   // u.reflection_color == nullptr; a frame in flight keeps reading the old canvas, which stays allocated
        ctx->rt_have_refl = false;
        return SHS_OK;
    }
    if (w <= 0 || h <= 0 || w > 32767 || h > 32767) {
        ctx->err = "shs_rt_set_reflection: 1 .. 32767 per side";
        return SHS_ERR_INVALID;
    }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t npx = (size_t)w * h;
    ctx->rt_have_refl = false;
    if (ensure(ctx, ctx->rt_refl, npx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->rt_refl.p, rgba, npx * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the pageable staging is consumed by now)
    ctx->rt_refl_w = w;
    ctx->rt_refl_h = h;
    ctx->rt_have_refl = true;
    return SHS_OK;
}

int shs_rt_water_samples(shs_ctx *ctx, int32_t n, const float *world_pos3, float time_sec, float *normal3, float *foam) {
    if (!ctx || n < 0 || (n > 0 && (!world_pos3 || !normal3 || !foam))) return SHS_ERR_INVALID;
    if (!std::isfinite(time_sec)) {
        ctx->err = "shs_rt_water_samples: a non-finite time_sec";
        return SHS_ERR_INVALID;
    }
    if (n == 0) return SHS_OK;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t ns = (size_t)n;
    if (ensure(ctx, ctx->rt_water_io, 7 * ns)) return SHS_ERR_HIP;   // the workspace: points (3 n), normals (3 n), foam (n)
    float *io = ctx->rt_water_io.p;
    HIP_TRY(ctx, hipMemcpyAsync(io, world_pos3, 3 * ns * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    shs_dev::RtWaterSamples q{};
    q.n = n;
    q.world = io;
    q.normal = io + 3 * ns;
    q.foam = io + 6 * ns;
    q.water = water_model(time_sec);
    HIP_TRY(ctx, shs_internal::launch_water_samples(q, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(normal3, q.normal, 3 * ns * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(foam, q.foam, ns * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the pageable staging above is consumed by now)
    return SHS_OK;
}

int shs_rt_resolve(shs_ctx *ctx, uint8_t *color, float *depth, float *velocity) {
    if (!ctx || !ctx->rt_have_frame) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t npx = (size_t)ctx->rt_w * ctx->rt_h;
    if (color) HIP_TRY(ctx, hipMemcpyAsync(color, ctx->rt_color.p, npx * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (depth) HIP_TRY(ctx, hipMemcpyAsync(depth, ctx->rt_depth.p, npx * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (velocity) HIP_TRY(ctx, hipMemcpyAsync(velocity, ctx->rt_vel.p, npx * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SHS_OK;
}

int shs_rt_resolve_shadow(shs_ctx *ctx, float *shadow_map) {
    if (!ctx || !shadow_map || !ctx->rt_have_shadow) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(shadow_map, ctx->rt_shadow.p, (size_t)ctx->rt_sw * ctx->rt_sh * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SHS_OK;
}

int shs_rt_resolve_prequant(shs_ctx *ctx, float *prequant) {
    if (!ctx || !prequant || !ctx->rt_have_frame || !ctx->rt_have_pq) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(prequant, ctx->rt_pq.p, (size_t)ctx->rt_w * ctx->rt_h * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SHS_OK;
}

int shs_rt_resolve_ids(shs_ctx *ctx, int32_t *tri_id) {
    if (!ctx || !tri_id || !ctx->rt_have_frame) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(tri_id, ctx->rt_ids.p, (size_t)ctx->rt_w * ctx->rt_h * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SHS_OK;
}

int shs_rt_get_stats(shs_ctx *ctx, shs_rt_stats *st) {
    if (!ctx || !st || !ctx->rt_have_frame) return SHS_ERR_INVALID;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(h, ctx->rt_stats.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    st->input_tris = ctx->rt_n_tris;
    st->polys3 = (int64_t)h[1];
    st->polys4 = (int64_t)h[2];
    st->sub_tris = (int64_t)h[3];
    return SHS_OK;
}

int shs_rt_device_targets(shs_ctx *ctx, void **color_dev, void **depth_dev, void **velocity_dev) {
    if (!ctx || !ctx->rt_have_frame) return SHS_ERR_INVALID;
    // the passes are enqueued whole on the context stream: the planes are final in its order
    if (color_dev) *color_dev = ctx->rt_color.p;
    if (depth_dev) *depth_dev = ctx->rt_depth.p;
    if (velocity_dev) *velocity_dev = ctx->rt_vel.p;
    return SHS_OK;
}

int shs_rt_device_shadow_map(shs_ctx *ctx, void **map_dev, int32_t *w, int32_t *h) {
    if (!ctx || !ctx->rt_have_shadow) return SHS_ERR_INVALID;
    if (map_dev) *map_dev = ctx->rt_shadow.p;
    if (w) *w = ctx->rt_sw;
    if (h) *h = ctx->rt_sh;
    return SHS_OK;
}

int shs_rt_set_pcss(shs_ctx *ctx, const shs_rt_pcss *pcss) {
    if (!ctx) return SHS_ERR_INVALID;
    const shs_rt_pcss demo = {0.0035f, 18.0f, 1.0f, 28.0f, 1e-5f, 12, 24};
    if (pcss && !pcss_ok(*pcss)) {
        ctx->err = "shs_rt_set_pcss: a non-finite constant or a sample count outside 0..64";
        return SHS_ERR_INVALID;
    }
    ctx->rt_pcss = pcss ? *pcss : demo;
    return SHS_OK;
}

int shs_rt_pcss_samples(shs_ctx *ctx, const float *map, int32_t w, int32_t h, int32_t n, const float *uv, const float *z,
                        const float *bias, const int32_t *pxpy, float *out) {
    if (!ctx || !map || w <= 0 || h <= 0 || w > 32767 || h > 32767 || n < 0 || (n > 0 && (!uv || !z || !bias || !pxpy || !out)))
        return SHS_ERR_INVALID;
    if (n == 0) return SHS_OK;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t nm = (size_t)w * h, ns = (size_t)n;
    // the workspace: uv (2 n), z (n), bias (n), out (n)
    if (ensure(ctx, ctx->rt_ps_map, nm) || ensure(ctx, ctx->rt_ps_io, 5 * ns) || ensure(ctx, ctx->rt_ps_rot, ns)) return SHS_ERR_HIP;
    std::vector<float> rot(4 * ns);
    for (size_t i = 0; i < ns; ++i) pixel_rotation(pxpy[2 * i], pxpy[2 * i + 1], &rot[4 * i]);
    float *io = ctx->rt_ps_io.p;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->rt_ps_map.p, map, nm * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(io, uv, 2 * ns * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(io + 2 * ns, z, ns * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(io + 3 * ns, bias, ns * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->rt_ps_rot.p, rot.data(), ns * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    shs_dev::RtPcssSamples q{};
    q.map = ctx->rt_ps_map.p;
    q.w = w; q.h = h; q.n = n;
    q.uv = io;
    q.z = io + 2 * ns;
    q.bias = io + 3 * ns;
    q.rot = ctx->rt_ps_rot.p;
    q.out = io + 4 * ns;
    fill_pcss(q, ctx->rt_pcss);
    HIP_TRY(ctx, shs_internal::launch_pcss_samples(q, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out, q.out, ns * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the pageable staging above is consumed by now)
    return SHS_OK;
}

int shs_rt_set_pbr(shs_ctx *ctx, const shs_rt_pbr *pbr) {
    if (!ctx) return SHS_ERR_INVALID;
    const shs_rt_pbr demo = {1.75f, 0.04f, 3.0f};
    if (pbr && !(std::isfinite(pbr->exposure) && std::isfinite(pbr->min_roughness) && std::isfinite(pbr->direct_intensity))) {
        ctx->err = "shs_rt_set_pbr: a non-finite constant";
        return SHS_ERR_INVALID;
    }
    ctx->rt_pbr = pbr ? *pbr : demo;
    return SHS_OK;
}

int shs_rt_set_ibl(shs_ctx *ctx, int32_t irr_size, const float *irr, int32_t spec_base, int32_t mip_count, const float *spec) {
    if (!ctx) return SHS_ERR_INVALID;
    if (!irr) {   // u.ibl == nullptr; a frame in flight keeps reading the old levels, which stay allocated
        ctx->rt_ibl_mips = 0;
        return SHS_OK;
    }
    if (irr_size <= 0 || spec_base <= 0 || mip_count < 1 || mip_count > 16 || !spec || irr_size > 8192 || spec_base > 8192) {
        ctx->err = "shs_rt_set_ibl: sizes 1 .. 8192, 1 .. 16 mips, both maps given";
        return SHS_ERR_INVALID;
    }
    // the level table, then the texels padded to float4 (shs_canvas_rt_internal.hpp)
    int32_t size[shs_dev::RT_IBL_LEVELS] = {irr_size};
    size_t total = shs_dev::RT_IBL_LEVELS;
    std::vector<float4> host(total);
    for (int l = 0; l <= mip_count; ++l) {
        if (l > 0) size[l] = std::max(1, spec_base >> (l - 1));   // ibl.hpp:168
        const int32_t hd[4] = {(int32_t)total, size[l], 0, 0};
        std::memcpy(&host[l], hd, sizeof hd);
        total += (size_t)6 * size[l] * size[l];
    }
    if (total > ((size_t)1 << 27)) {
        ctx->err = "shs_rt_set_ibl: more than 2^27 texels";
        return SHS_ERR_INVALID;
    }
    host.resize(total);
    size_t o = shs_dev::RT_IBL_LEVELS;
    const float *src = irr;
    for (int l = 0; l <= mip_count; ++l) {
        if (l == 1) src = spec;
        const size_t n = (size_t)6 * size[l] * size[l];
        for (size_t i = 0; i < n; ++i) host[o + i] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], 0.0f);
        o += n;
        src += 3 * n;
    }
    if (set_dev(ctx)) return SHS_ERR_HIP;
    // a camera pass in flight may still read the levels: finish it before they are overwritten
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->rt_ibl_mips = 0;
    if (ensure(ctx, ctx->rt_ibl, total)) return SHS_ERR_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->rt_ibl.p, host.data(), total * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the pageable staging is consumed by now)
    ctx->rt_ibl_mips = mip_count;
    return SHS_OK;
}

int shs_rt_ibl_samples(shs_ctx *ctx, int32_t n, const float *dirs3, const float *lod, float *irr_rgb3, float *spec_rgb3) {
    if (!ctx || n < 0 || (n > 0 && (!dirs3 || !lod || !irr_rgb3 || !spec_rgb3))) return SHS_ERR_INVALID;
    if (ctx->rt_ibl_mips <= 0) {
        ctx->err = "shs_rt_ibl_samples: no IBL set (shs_rt_set_ibl)";
        return SHS_ERR_INVALID;
    }
    if (n == 0) return SHS_OK;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t ns = (size_t)n;
    // the workspace: dirs (3 n), lod (n), irradiance (3 n), specular (3 n)
    if (ensure(ctx, ctx->rt_is_io, 10 * ns)) return SHS_ERR_HIP;
    float *io = ctx->rt_is_io.p;
    HIP_TRY(ctx, hipMemcpyAsync(io, dirs3, 3 * ns * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(io + 3 * ns, lod, ns * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    shs_dev::RtIblSamples q{};
    q.ibl = ctx->rt_ibl.p;
    q.ibl_mips = ctx->rt_ibl_mips;
    q.n = n;
    q.dirs = io;
    q.lod = io + 3 * ns;
    q.irr = io + 4 * ns;
    q.spec = io + 7 * ns;
    HIP_TRY(ctx, shs_internal::launch_ibl_samples(q, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(irr_rgb3, q.irr, 3 * ns * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(spec_rgb3, q.spec, 3 * ns * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the pageable staging above is consumed by now)
    return SHS_OK;
}

int shs_rt_set_sky(shs_ctx *ctx, const shs_rt_sky *sky) {
    if (!ctx) return SHS_ERR_INVALID;
    if (!sky || sky->model == SHS_RT_SKY_NONE) {
        ctx->rt_sky = shs_rt_sky{};
        return SHS_OK;
    }
    const bool cube = sky->model == SHS_RT_SKY_CUBEMAP;
    if ((sky->model != SHS_RT_SKY_ANALYTIC && !cube) || (sky->encode != SHS_RT_SKY_ENCODE_REINHARD && sky->encode != SHS_RT_SKY_ENCODE_CLAMP)) {
        ctx->err = "shs_rt_set_sky: unknown model or encode";
        return SHS_ERR_INVALID;
    }
    bool fin = std::isfinite(sky->intensity) && std::isfinite(sky->fov_degrees) && std::isfinite(sky->exposure);
    for (int k = 0; k < 3; ++k)
        fin = fin && std::isfinite(sky->sun_dir[k]) && std::isfinite(sky->cam_forward[k]) && std::isfinite(sky->cam_right[k]) &&
              std::isfinite(sky->cam_up[k]);
    if (!fin) {
        ctx->err = "shs_rt_set_sky: a non-finite float";
        return SHS_ERR_INVALID;
    }
    using shs_host::vec3;
    auto finite3 = [](vec3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); };
    // glm::normalize of the three camera vectors (pbr :746-748) and the pass's tangent (:744), once per call
    const vec3 cam[3] = {shs_host::gnormalize({sky->cam_forward[0], sky->cam_forward[1], sky->cam_forward[2]}),
                         shs_host::gnormalize({sky->cam_right[0], sky->cam_right[1], sky->cam_right[2]}),
                         shs_host::gnormalize({sky->cam_up[0], sky->cam_up[1], sky->cam_up[2]})};
    const float tan_half_fov = std::tan(shs_host::gradians(sky->fov_degrees) * 0.5f);
    if (!finite3(cam[0]) || !finite3(cam[1]) || !finite3(cam[2]) || !std::isfinite(tan_half_fov)) {
        ctx->err = "shs_rt_set_sky: a camera vector that cannot be normalised";
        return SHS_ERR_INVALID;
    }
    shs_dev::RtSkyModel m{};
    if (cube) {
        for (int k = 0; k < 6; ++k) {
            const int32_t id = sky->face_tex[k];
            if (id <= 0 || id > (int32_t)ctx->textures.size() || !ctx->textures[(size_t)id - 1].live) {
                ctx->err = "shs_rt_set_sky: unknown face texture id";
                return SHS_ERR_INVALID;
            }
            const Texture &t = ctx->textures[(size_t)id - 1];
            m.face[k] = t.texels;
            m.fw[k] = t.w;
            m.fh[k] = t.h;
        }
        m.intensity = sky->intensity;
        if (set_dev(ctx)) return SHS_ERR_HIP;
        if (ensure_srgb_table(ctx)) return SHS_ERR_HIP;   // (the first cubemap sky of a context uploads the table)
        m.srgb_lut = ctx->rt_srgb_lut.p;
    } else {
        // AnalyticSky::sample's terms of the sun direction alone (shs_renderer.hpp:561, :568-579, :589, :596), each a
        // single float operation in the reference's order; glm::mix(x, y, a) is x * (1 - a) + y * a
        const vec3 s = shs_host::gneg(shs_host::gnormalize({sky->sun_dir[0], sky->sun_dir[1], sky->sun_dir[2]}));
        if (!finite3(s)) {
            ctx->err = "shs_rt_set_sky: a sun direction that cannot be normalised";
            return SHS_ERR_INVALID;
        }
        const float lo = (s.y < 0.0f) ? 0.0f : s.y;             // glm::clamp(s.y, 0, 1): min(max(x, 0), 1)
        const float sun_height = (1.0f < lo) ? 1.0f : lo;
        const float a = sun_height, b = 1.0f - sun_height;
        const float zenith_night[3] = {0.02f, 0.02f, 0.05f}, zenith_day[3] = {0.30f, 0.70f, 1.70f};
        const float horizon_night[3] = {0.4f, 0.15f, 0.05f}, horizon_day[3] = {1.30f, 1.64f, 2.00f};
        const float ground_base[3] = {0.30f, 0.26f, 0.22f}, glow_base[3] = {1.0f, 0.8f, 0.4f};
        m.s[0] = s.x; m.s[1] = s.y; m.s[2] = s.z;
        for (int k = 0; k < 3; ++k) {
            m.zenith[k] = zenith_night[k] * b + zenith_day[k] * a;
            m.horizon[k] = horizon_night[k] * b + horizon_day[k] * a;
            const float half_ground = ground_base[k] * 0.5f;
            const float ground = half_ground * b + ground_base[k] * a;
            const float reflected = m.horizon[k] * 0.05f;
            m.ground[k] = ground + reflected;
            m.half_horizon[k] = m.horizon[k] * 0.5f;
            const float glow4 = glow_base[k] * 4.0f;
            m.glow[k] = glow4 * sun_height;
        }
    }
    ctx->rt_sky = *sky;
    ctx->rt_sky_model = m;
    for (int k = 0; k < 3; ++k) {
        ctx->rt_sky_cam[3 * k] = cam[k].x;
        ctx->rt_sky_cam[3 * k + 1] = cam[k].y;
        ctx->rt_sky_cam[3 * k + 2] = cam[k].z;
    }
    ctx->rt_sky_tan = tan_half_fov;
    return SHS_OK;
}

int shs_rt_sky_samples(shs_ctx *ctx, int32_t n, const float *dirs3, float *rgb3) {
    if (!ctx || n < 0 || (n > 0 && (!dirs3 || !rgb3))) return SHS_ERR_INVALID;
    if (ctx->rt_sky.model == SHS_RT_SKY_NONE) {
        ctx->err = "shs_rt_sky_samples: no sky bound (shs_rt_set_sky)";
        return SHS_ERR_INVALID;
    }
    if (n == 0) return SHS_OK;
    if (set_dev(ctx)) return SHS_ERR_HIP;
    const size_t ns = (size_t)n;
    if (ensure(ctx, ctx->rt_sky_io, 6 * ns)) return SHS_ERR_HIP;   // the workspace: dirs (3 n), radiance (3 n)
    float *io = ctx->rt_sky_io.p;
    HIP_TRY(ctx, hipMemcpyAsync(io, dirs3, 3 * ns * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    shs_dev::RtSkySamples q{};
    q.n = n;
    q.dirs = io;
    q.out = io + 3 * ns;
    q.sky = ctx->rt_sky_model;
    HIP_TRY(ctx, shs_internal::launch_sky_samples(q, ctx->rt_sky.model, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(rgb3, q.out, 3 * ns * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the pageable staging above is consumed by now)
    return SHS_OK;
}

int shs_ortho_lh_zo(float left, float right, float bottom, float top, float znear, float zfar, float out16[16]) {
    if (!out16) return SHS_ERR_INVALID;
    shs_host::ortho_lh_zo(left, right, bottom, top, znear, zfar, out16);
    return SHS_OK;
}

}  // extern "C"
