// ref_lib.cpp -- driver that runs the REFERENCE LIBRARY'S OWN HEADERS behind the oracle's C ABI.
//
// TEST INFRASTRUCTURE ONLY.  Built by `make -C oracle ref` into oracle/_ref/libshs_ref_lib.so with
// the reference tree on the include path and oracle/glm_standin in place of GLM (see
// glm_standin/glm/glm.hpp: GLM itself stays unpinned).  Nothing of the reference and nothing compiled
// from it is committed; this file only names its headers.
//
// ref_pbr_forward / ref_tonemap / ref_motion_blur take the structs and argument lists of
// ora_pbr_forward / ora_tonemap / ora_motion_blur (shs_oracle.h), so tests/test_lib_reference*.py
// compare the oracle (and the GPU) with the compiled reference word for word.
#include <cstdint>
#include <cstring>
#include <vector>

#include "shs/core/context.hpp"
#include "shs/lighting/shadow_sample.hpp"
#include "shs/passes/pass_motion_blur.hpp"
#include "shs/passes/pass_tonemap.hpp"
#include "shs/shader/builtin_shaders.hpp"
#include "shs/sw_render/rasterizer.hpp"

#include "shs_oracle.h"

static_assert(sizeof(glm::vec2) == 8 && sizeof(glm::vec3) == 12 && sizeof(glm::vec4) == 16, "packed vectors");
static_assert(sizeof(glm::mat4) == 64, "column-major float[16]");
static_assert(sizeof(shs::ColorF) == 16 && sizeof(shs::Color) == 4 && sizeof(shs::Motion2f) == 8, "packed pixels");

namespace {

// The caller's matrix bytes, straight through (never rebuilt with a matrix builder).
glm::mat4 mat_of(const float *m) {
    glm::mat4 o;
    std::memcpy(&o, m, sizeof o);
    return o;
}

glm::vec3 vec_of(const float *v) { return glm::vec3(v[0], v[1], v[2]); }

// ora_mesh -> MeshData; normal / uv arrays shorter than the positions stay short (read_v's defaults).
void fill_mesh(const ora_mesh &m, shs::MeshData &out) {
    out.positions.resize((size_t)(m.n_verts > 0 ? m.n_verts : 0));
    if (!out.positions.empty()) std::memcpy(out.positions.data(), m.positions, out.positions.size() * sizeof(glm::vec3));
    out.normals.resize(m.normals && m.n_normals > 0 ? (size_t)m.n_normals : 0);
    if (!out.normals.empty()) std::memcpy(out.normals.data(), m.normals, out.normals.size() * sizeof(glm::vec3));
    out.uvs.resize(m.uvs && m.n_uvs > 0 ? (size_t)m.n_uvs : 0);
    if (!out.uvs.empty()) std::memcpy(out.uvs.data(), m.uvs, out.uvs.size() * sizeof(glm::vec2));
    if (m.indices && m.n_indices > 0) out.indices.assign(m.indices, m.indices + m.n_indices);
}

}  // namespace

extern "C" {

int ref_pbr_forward(const ora_lib_target *t, const ora_lib_draw *draws, int n_draws, uint64_t *stats3) {
    if (!t || !t->hdr || t->W <= 0 || t->H <= 0 || (n_draws > 0 && !draws)) return -1;
    for (int i = 0; i < n_draws; ++i)
        if (draws[i].program < ORA_PROGRAM_PBR_MR || draws[i].program > ORA_PROGRAM_DEBUG_DEPTH) return -2;
    const int W = t->W, H = t->H;

    // The pass's clears in our own words (as ora_pbr_forward): each row of the HDR target gets the
    // no-sky gradient at tt = y / max(1, H - 1), or the clear colour; depth 1, motion 0.
    shs::RT_ColorHDR hdr(W, H);
    for (int y = 0; y < H; ++y) {
        shs::ColorF c;
        if (t->bg_gradient) {
            const float tt = (float)y / (float)(H - 1 > 1 ? H - 1 : 1);
            c = shs::ColorF{0.06f + 0.08f * tt, 0.08f + 0.10f * tt, 0.12f + 0.12f * tt, 1.0f};
        } else {
            c = shs::ColorF{t->clear_hdr[0], t->clear_hdr[1], t->clear_hdr[2], t->clear_hdr[3]};
        }
        for (int x = 0; x < W; ++x) hdr.color.at(x, y) = c;
    }
    shs::RT_ColorDepthMotion dm;
    if (t->depth) dm = shs::RT_ColorDepthMotion(W, H, t->zn, t->zf);
    shs::RT_ShadowDepth sm;
    if (t->shadow && t->shadow_w > 0 && t->shadow_h > 0) {
        sm.resize(t->shadow_w, t->shadow_h);
        std::memcpy(sm.data(), t->shadow, sizeof(float) * (size_t)t->shadow_w * (size_t)t->shadow_h);
    }

    shs::RasterizerTarget target{};
    target.hdr = &hdr;
    target.depth_motion = t->depth ? &dm : nullptr;

    stats3[0] = stats3[1] = stats3[2] = 0;
    for (int i = 0; i < n_draws; ++i) {
        const ora_lib_draw &d = draws[i];
        shs::MeshData mesh{};
        fill_mesh(d.mesh, mesh);
        shs::Texture2DData tex{};
        if (d.base_color_tex && d.tex_w > 0 && d.tex_h > 0) {
            tex = shs::Texture2DData(d.tex_w, d.tex_h);
            std::memcpy(tex.texels.data(), d.base_color_tex, tex.texels.size() * sizeof(shs::Color));
        }

        shs::ShaderUniforms u{};
        u.model = mat_of(d.model);
        u.viewproj = mat_of(d.viewproj);
        u.prev_model = mat_of(d.prev_model);
        u.prev_viewproj = mat_of(d.prev_viewproj);
        u.light_dir_ws = vec_of(d.light_dir_ws);
        u.light_color = vec_of(d.light_color);
        u.light_intensity = d.light_intensity;
        u.camera_pos = vec_of(d.camera_pos);
        u.base_color = vec_of(d.base_color);
        u.metallic = d.metallic;
        u.roughness = d.roughness;
        u.ao = d.ao;
        u.base_color_tex = tex.valid() ? &tex : nullptr;
        u.shadow_map = (d.shadow && sm.w > 0) ? &sm : nullptr;
        u.light_viewproj = mat_of(d.light_viewproj);
        u.shadow_bias_const = d.shadow_bias_const;
        u.shadow_bias_slope = d.shadow_bias_slope;
        u.shadow_pcf_radius = d.shadow_pcf_radius;
        u.shadow_pcf_step = d.shadow_pcf_step;
        u.shadow_strength = d.shadow_strength;
        u.enable_motion_vectors = d.enable_motion_vectors != 0;

        shs::ShaderProgram program;
        switch (d.program) {
            case ORA_PROGRAM_PBR_MR: program = shs::make_pbr_mr_program(); break;
            case ORA_PROGRAM_BLINN_PHONG: program = shs::make_blinn_phong_program(); break;
            case ORA_PROGRAM_DEBUG_ALBEDO: program = shs::make_debug_view_shader_program(shs::DebugViewMode::Albedo); break;
            case ORA_PROGRAM_DEBUG_NORMAL: program = shs::make_debug_view_shader_program(shs::DebugViewMode::Normal); break;
            default: program = shs::make_debug_view_shader_program(shs::DebugViewMode::Depth); break;
        }

        shs::RasterizerConfig cfg{};
        cfg.cull_mode = (shs::RasterizerCullMode)d.cull_mode;
        cfg.front_face_ccw = d.front_face_ccw != 0;
        cfg.job_system = nullptr;

        const shs::RasterizerStats st = shs::rasterize_mesh(mesh, program, u, target, cfg);
        stats3[0] += st.tri_input;
        stats3[1] += st.tri_after_clip;
        stats3[2] += st.tri_raster;
    }

    std::memcpy(t->hdr, hdr.color.data.data(), sizeof(float) * 4 * (size_t)W * (size_t)H);
    if (t->depth) std::memcpy(t->depth, dm.depth.data.data(), sizeof(float) * (size_t)W * (size_t)H);
    if (t->depth && t->motion) std::memcpy(t->motion, dm.motion.data.data(), sizeof(float) * 2 * (size_t)W * (size_t)H);
    return 0;
}

// PassTonemap::execute; the `present` plane of ora_tonemap is not the reference library's (it belongs
// to a demo's upload helper), so only ldr is written.
void ref_tonemap(const float *hdr, int W, int H, float exposure, float gamma, uint8_t *ldr, uint8_t *present) {
    (void)present;
    if (!hdr || !ldr || W <= 0 || H <= 0) return;
    shs::RT_ColorHDR in(W, H);
    std::memcpy(in.color.data.data(), hdr, sizeof(float) * 4 * (size_t)W * (size_t)H);
    shs::RT_ColorLDR out(W, H);
    shs::FrameParams fp{};
    fp.w = W;
    fp.h = H;
    fp.pass.tonemap.exposure = exposure;
    fp.pass.tonemap.gamma = gamma;
    shs::RTRegistry reg;
    shs::PassTonemap::Inputs io{};
    io.fp = &fp;
    io.rtr = &reg;
    io.rt_hdr = reg.reg<shs::RTHandle>(&in);
    io.rt_ldr = reg.reg<shs::RTHandle>(&out);
    shs::Context ctx{};
    shs::PassTonemap pass;
    pass.execute(ctx, io);
    std::memcpy(ldr, out.color.data.data(), 4 * (size_t)W * (size_t)H);
}

void ref_motion_blur(const uint8_t *src, const float *depth, const float *motion, int W, int H, int enable,
                     int samples, float strength, float max_velocity_px, float min_velocity_px, float depth_reject,
                     float dt, uint8_t *dst) {
    if (!src || !depth || !motion || !dst || W <= 0 || H <= 0) return;
    const size_t n = (size_t)W * (size_t)H;
    shs::RT_ColorLDR in(W, H), out(W, H);
    std::memcpy(in.color.data.data(), src, 4 * n);
    shs::RT_ColorDepthMotion dm(W, H, 0.1f, 1000.0f);
    std::memcpy(dm.depth.data.data(), depth, sizeof(float) * n);
    std::memcpy(dm.motion.data.data(), motion, sizeof(float) * 2 * n);
    shs::FrameParams fp{};
    fp.w = W;
    fp.h = H;
    fp.dt = dt;
    fp.pass.motion_blur.enable = enable != 0;
    fp.pass.motion_blur.samples = samples;
    fp.pass.motion_blur.strength = strength;
    fp.pass.motion_blur.max_velocity_px = max_velocity_px;
    fp.pass.motion_blur.min_velocity_px = min_velocity_px;
    fp.pass.motion_blur.depth_reject = depth_reject;
    shs::RTRegistry reg;
    shs::PassMotionBlur::Inputs io{};
    io.fp = &fp;
    io.rtr = &reg;
    io.rt_input_ldr = reg.reg<shs::RTHandle>(&in);
    io.rt_output_ldr = reg.reg<shs::RTHandle>(&out);
    io.rt_motion = reg.reg<shs::RTHandle>(&dm);
    shs::Context ctx{};
    shs::PassMotionBlur pass;
    pass.execute(ctx, io);
    std::memcpy(dst, out.color.data.data(), 4 * n);
}

}  // extern "C"
