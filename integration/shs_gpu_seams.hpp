// shs_gpu_seams.hpp -- drop-in adapters that route the reference's hot path through libshs_gpu.
//
// Header-only C++20 for the reference tree (sharavsambuu/leisure-software-renderer); it includes the
// reference's own headers and glm, so it compiles there, not in this repository's image (glm, SDL2
// and assimp are absent here -- SURVEY.md 8c).  The C ABI it calls (include/shs_gpu.h) is compiled
// and exercised here by tests/abi_c/abi_legacy.cpp.  Paths below are relative to
// /root/reference/cpp-folders/src/.
//
//   Seam 1  LegacyRendererSystemGPU<SceneT, ObjectT, SHADING>: replaces RendererSystem of
//           hello-3d-primitives/hello_pipeline_{blinn_phong,phong,gouraud,flat,toon,gooch,oren_nayar}_shading.cpp
//           and hello_pipeline_texture_mapping.cpp
//           (the 80x80 tile-job loop of process(), :244-313 in the Blinn-Phong demo), and with three
//           draws per object the split-screen hello_pipeline_normal_zbuffer_debug.cpp.
//   Seam 1b RenderTargetSystemGPU<SceneT>: the Canvas render-target raster of
//           hello-render-target/hello_shadow_mapping.cpp (PASS0 shadow map, PASS1 colour + depth + velocity
//           with the shadow lookup; shs_rt_*), its planes handed on the device to shs_canvas_motion_blur.
//   Seam 3  PassShadowMapGPU / PassPBRForwardGPU: IRenderPass implementations with the ids,
//           contracts and resource I/O of PassShadowMapAdapter / PassPBRForwardAdapter
//           (shs-renderer-lib/include/shs/pipeline/pass_adapters.hpp:356-394, 1005-1062), registered
//           under "shadow_map" / "pbr_forward" by register_gpu_passes() over the standard registry
//           (make_standard_pass_factory_registry, pass_adapters.hpp:1497-1568).
#pragma once

#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include <glm/glm.hpp>
#include <glm/gtc/matrix_transform.hpp>
#include <glm/gtc/type_ptr.hpp>

#include "shs_gpu.h"

namespace shs_gpu_seams {

inline void check(shs_ctx *ctx, int rc) {
    if (rc != SHS_OK) throw std::runtime_error(ctx ? shs_last_error(ctx) : "shs_gpu: no context");
}

// One device context per host render thread (a context is used by one thread).
struct Device {
    shs_ctx *ctx = nullptr;
    explicit Device(int device_index = 0) {
        if (shs_create(device_index, &ctx) != SHS_OK) throw std::runtime_error("shs_gpu: no gfx950 device");
    }
    ~Device() { shs_destroy(ctx); }
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
};

// =====================================================================================================
// Seam 1 -- the legacy Canvas / ZBuffer / draw-call path.
//
// Maintainer edit in a hello_pipeline_*_shading.cpp demo (SystemProcessor, :327-360 of the Blinn-Phong
// demo): declare the member as `shs::AbstractSystem *renderer_system;` and construct
//     this->renderer_system = new shs_gpu_seams::LegacyRendererSystemGPU<HelloScene, MonkeyObject,
//                                                                      SHS_SHADING_BLINN_PHONG>(scene);
// (SHS_SHADING_PHONG / _GOURAUD / _FLAT in the other three demos; SHS_SHADING_TOON / _GOOCH /
// _OREN_NAYAR in hello_pipeline_{toon,gooch,oren_nayar}_shading.cpp, whose Uniforms and vertex shader
// are the Blinn-Phong demo's, as are SHS_SHADING_NORMAL_VIS / _DEPTH_VIS's; SHS_SHADING_TEXTURED in
// hello_pipeline_texture_mapping.cpp with ObjectT = SubaruObject, whose geometry->uvs and albedo are passed
// through -- process() sets use_texture whenever the object has a valid albedo, :336).  Everything else -- the scene,
// the LogicSystem / Viewer camera update, Canvas::fill_pixel, copy_to_SDLSurface and the SDL loop --
// is unchanged.  The job system is no longer used for rendering.
//
// SceneT must provide what RendererSystem reads (HelloScene, blinn_phong_shading.cpp:144-163):
//   std::vector<shs::AbstractObject3D*> scene_objects; shs::Canvas *canvas; shs::Viewer *viewer;
//   glm::vec3 light_direction;
// ObjectT (MonkeyObject, :110-141): ModelGeometry *geometry; shs::Color color; get_world_matrix().
// =====================================================================================================
template <class SceneT, class ObjectT, int SHADING>
class LegacyRendererSystemGPU : public shs::AbstractSystem {
public:
    static_assert(SHADING >= SHS_SHADING_FLAT && SHADING <= SHS_SHADING_TEXTURED, "a legacy shading model");
    static constexpr int kTileX = 80, kTileY = 80;   // TILE_SIZE_X / _Y (blinn_phong_shading.cpp:29-30)

    explicit LegacyRendererSystemGPU(SceneT *scene, int device_index = 0)
        : scene_(scene), dev_(device_index),
          // the same ZBuffer RendererSystem allocates in its constructor (:176-181)
          z_buffer_(scene->canvas->get_width(), scene->canvas->get_height(), scene->viewer->camera->z_near,
                    scene->viewer->camera->z_far) {}

    // RendererSystem::process(dt) (:244-313): clear z, rasterise every object, join -- one enqueue plus
    // one resolve into the caller-owned Canvas / ZBuffer in their own layouts.
    void process(float /*delta_time*/) override {
        shs::Canvas &canvas = *scene_->canvas;
        const glm::mat4 view = scene_->viewer->camera->view_matrix;
        const glm::mat4 proj = scene_->viewer->camera->projection_matrix;
        // flat_shading.cpp:256: the Flat pipeline's view-space light direction
        const glm::vec3 light_dir_view = glm::normalize(glm::vec3(view * glm::vec4(scene_->light_direction, 0.0f)));

        draws_.clear();
        albedo_.clear();
        for (shs::AbstractObject3D *object : scene_->scene_objects) {
            auto *obj = dynamic_cast<ObjectT *>(object);   // the demo's `if (!monkey) continue;`
            if (!obj) continue;
            shs_legacy_draw d{};
            d.mesh_id = mesh_id(obj);
            d.shading = SHADING;
            if constexpr (SHADING == SHS_SHADING_FLAT) {
                // Uniforms{mv, mvp, light_dir_view, color} (flat_shading.cpp:284-287)
                const glm::mat4 mv = view * obj->get_world_matrix();
                const glm::mat4 mvp = proj * mv;
                std::memcpy(d.mvp, glm::value_ptr(mvp), sizeof d.mvp);
                std::memcpy(d.model, glm::value_ptr(mv), sizeof d.model);
                std::memcpy(d.light_dir, glm::value_ptr(light_dir_view), sizeof d.light_dir);
            } else {
                // Uniforms{model, mvp = proj * view * model, light_dir, camera_pos, color} (:277-282; the
                // same block in the Toon, Gooch, Oren-Nayar and split-screen demos)
                const glm::mat4 model = obj->get_world_matrix();
                const glm::mat4 mvp = proj * view * model;
                std::memcpy(d.mvp, glm::value_ptr(mvp), sizeof d.mvp);
                std::memcpy(d.model, glm::value_ptr(model), sizeof d.model);
                std::memcpy(d.light_dir, glm::value_ptr(scene_->light_direction), sizeof d.light_dir);
                std::memcpy(d.camera_pos, glm::value_ptr(scene_->viewer->position), sizeof d.camera_pos);
            }
            d.color[0] = obj->color.r; d.color[1] = obj->color.g; d.color[2] = obj->color.b; d.color[3] = obj->color.a;
            draws_.push_back(d);
            // Uniforms::albedo / use_texture (texture_mapping.cpp:56-57): the object's texture, 0 without one
            if constexpr (SHADING == SHS_SHADING_TEXTURED) albedo_.push_back(texture_id(obj->albedo));
        }

        shs_frame_desc f{};
        f.width = canvas.get_width();
        f.height = canvas.get_height();
        f.ref_tile_w = kTileX;   // the reference's tile-clamp pixels are reproduced exactly
        f.ref_tile_h = kTileY;
        f.shard_rank = 0;
        f.shard_count = 1;
        // main() clears the canvas black before render (:441, Canvas::fill_pixel); the GPU frame
        // writes every pixel, clear included
        f.clear_color[0] = 0; f.clear_color[1] = 0; f.clear_color[2] = 0; f.clear_color[3] = 255;
        check(dev_.ctx, shs_render_legacy_batch_tex(dev_.ctx, &f, draws_.data(), albedo_.empty() ? nullptr : albedo_.data(),
                                                    static_cast<int32_t>(draws_.size()), 1));
        // Canvas::buffer() (Buffer<Color>, canvas rows bottom-up, RGBA8 -- shs_renderer.hpp:308-342, 753-796)
        // and ZBuffer::buffer() (screen rows as the legacy pipelines index it, :652-702)
        check(dev_.ctx, shs_resolve(dev_.ctx, reinterpret_cast<uint8_t *>(canvas.buffer().raw()), z_buffer_.buffer().raw()));
    }

    shs::ZBuffer &z_buffer() { return z_buffer_; }   // RendererSystem keeps it private; exposed here
    shs_ctx *context() { return dev_.ctx; }

private:
    // ModelGeometry's soup (shs_renderer.hpp:1296-1298): triangles[i] / normals[i], 3 corners per
    // triangle; uploaded once per geometry and kept device resident.
    int32_t mesh_id(ObjectT *obj) {
        auto it = mesh_ids_.find(obj->geometry);
        if (it != mesh_ids_.end()) return it->second;
        const auto &tri = obj->geometry->triangles;
        const auto &nrm = obj->geometry->normals;
        static_assert(sizeof(glm::vec3) == 12, "ModelGeometry vectors are packed float triples");
        int32_t id = -1;
        if constexpr (SHADING == SHS_SHADING_TEXTURED) {
            // the third stream, ModelGeometry::uvs (one vec2 per corner; vec2(0) where the file has none)
            const auto &uvs = obj->geometry->uvs;
            static_assert(sizeof(glm::vec2) == 8, "ModelGeometry::uvs are packed float pairs");
            check(dev_.ctx, shs_mesh_upload_soup_uv(dev_.ctx, glm::value_ptr(tri[0]), glm::value_ptr(nrm[0]),
                                                    uvs.size() == tri.size() ? glm::value_ptr(uvs[0]) : nullptr,
                                                    static_cast<int32_t>(tri.size() / 3), &id));
        } else {
            check(dev_.ctx, shs_mesh_upload_soup(dev_.ctx, glm::value_ptr(tri[0]), glm::value_ptr(nrm[0]),
                                                 static_cast<int32_t>(tri.size() / 3), &id));
        }
        mesh_ids_.emplace(obj->geometry, id);
        return id;
    }

    // A Texture2D (shs_renderer.hpp:351-364) as it stands after the host's loader: texels.raw() is w * h
    // Colors, texel (x, y) at y * w + x.  Uploaded once per texture; 0 (Uniforms::color) when there is none.
    int32_t texture_id(const shs::Texture2D *tex) {
        if (!tex || !tex->valid()) return 0;
        auto it = tex_ids_.find(tex);
        if (it != tex_ids_.end()) return it->second;
        static_assert(sizeof(shs::Color) == 4, "Texture2D::texels are RGBA8");
        int32_t id = 0;
        check(dev_.ctx, shs_texture_upload(dev_.ctx, reinterpret_cast<const uint8_t *>(tex->texels.raw()), tex->w, tex->h, &id));
        tex_ids_.emplace(tex, id);
        return id;
    }

    SceneT *scene_;
    Device dev_;
    shs::ZBuffer z_buffer_;
    std::vector<shs_legacy_draw> draws_;
    std::vector<int32_t> albedo_;   // SHS_SHADING_TEXTURED: parallel to draws_
    std::unordered_map<const void *, int32_t> mesh_ids_;
    std::unordered_map<const void *, int32_t> tex_ids_;
};

// -----------------------------------------------------------------------------------------------------
// Seam 1b -- the Canvas render-target raster (hello-render-target/hello_shadow_mapping.cpp).
//
// Replaces RendererSystem::process there (:1320-1600): PASS0 (shadow map), PASS1 (colour + view-z depth +
// velocity with the shadow lookup) and PASS2 (combined_motion_blur_pass) run on the device; only the final
// colours come back.  SceneT is that file's DemoScene (floor, car, monkey, viewer, canvas).  Uncompiled, like
// the other seams.
// -----------------------------------------------------------------------------------------------------
template <class SceneT>
class RenderTargetSystemGPU : public shs::AbstractSystem {
public:
    struct Object {
        int32_t mesh_id;             // shs_mesh_upload_soup_uv of the ModelGeometry / FloorPlane soup
        int32_t albedo_tex;          // shs_texture_upload id, 0: base_color
        shs::Color base_color;
        glm::mat4 model, prev_model;
    };

    RenderTargetSystemGPU(SceneT *scene, Device *dev, int shadow_size, int tile) : scene_(scene), dev_(dev), sm_(shadow_size), tile_(tile) {}

    std::vector<Object> objects;     // filled once by the host after its uploads; model / prev_model per frame

    void process(float) override {
        shs::Canvas &canvas = *scene_->canvas;
        const int W = canvas.get_width(), H = canvas.get_height();
        const glm::mat4 view = scene_->viewer->camera->view_matrix, proj = scene_->viewer->camera->projection_matrix;
        std::vector<shs_rt_draw> draws(objects.size());
        for (size_t i = 0; i < objects.size(); ++i) {
            const Object &o = objects[i];
            shs_rt_draw &d = draws[i];
            d.mesh_id = o.mesh_id;
            d.albedo_tex = o.albedo_tex;
            const glm::mat4 mvp = proj * view * o.model, prev_mvp = prev_vp_ * o.prev_model;
            std::memcpy(d.model, glm::value_ptr(o.model), 64);
            std::memcpy(d.mvp, glm::value_ptr(mvp), 64);
            std::memcpy(d.prev_mvp, glm::value_ptr(prev_mvp), 64);
            d.base_color[0] = o.base_color.r; d.base_color[1] = o.base_color.g; d.base_color[2] = o.base_color.b; d.base_color[3] = 255;
        }
        ok(shs_rt_render_shadow(dev_->ctx, sm_, sm_, tile_, tile_, glm::value_ptr(light_vp), draws.data(), (int32_t)draws.size()));
        shs_rt_frame f{};
        f.width = W; f.height = H; f.ref_tile_w = tile_; f.ref_tile_h = tile_;
        f.clear_color[0] = 20; f.clear_color[1] = 20; f.clear_color[2] = 25; f.clear_color[3] = 255;
        std::memcpy(f.view, glm::value_ptr(view), 64);
        std::memcpy(f.light_vp, glm::value_ptr(light_vp), 64);
        std::memcpy(f.light_dir_world, glm::value_ptr(light_dir_world), 12);
        std::memcpy(f.camera_pos, glm::value_ptr(scene_->viewer->position), 12);
        f.bias_base = 0.0025f; f.bias_slope = 0.01f; f.max_velocity_px = 22.0f;      // SHADOW_BIAS_*, MB_MAX_PIXELS
        f.flags = SHS_RT_USE_SHADOW | SHS_RT_PCF;
        ok(shs_rt_render(dev_->ctx, &f, draws.data(), (int32_t)draws.size()));
        void *color = nullptr, *depth = nullptr, *velocity = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &velocity));
        // PASS2 on the device (shs_canvas_motion_blur with SHS_CANVAS_DEVICE into a device buffer of the
        // host's), or shs_rt_resolve into rt->color / rt->depth / rt->velocity for a CPU PASS2.
        prev_vp_ = proj * view;
    }

    void ok(int rc) const {
        if (rc != SHS_OK) throw std::runtime_error(shs_last_error(dev_->ctx));
    }

    glm::mat4 light_vp{1.0f};        // light_proj * light_view (:1305-1317; shs_ortho_lh_zo, shs_look_at_lh)
    glm::vec3 light_dir_world{0.0f, -1.0f, 0.0f};

private:
    SceneT *scene_;
    Device *dev_;
    int sm_, tile_;
    glm::mat4 prev_vp_{1.0f};
};

// -----------------------------------------------------------------------------------------------------
// Seam 1b, soft -- hello-render-target/hello_shadow_mapping_soft.cpp.
//
// Replaces RendererSystem::process there (:1082-1400): the same two calls as the hard demo, with that file's tile
// jobs of 160 (TILE_SIZE_X / TILE_SIZE_Y :82-83) and shading = 1 (fragment_shader_softshadow :991-1040 over
// pcss_shadow_factor :333-445).  That demo has no motion buffer and no blur stage: prev_mvp is left zero, the
// velocity plane comes out zero and the colours are the frame.  The PCSS constants (:101-116) are the context's
// defaults; a host that changes them calls shs_rt_set_pcss once.  Uncompiled, like the other seams.
// -----------------------------------------------------------------------------------------------------
template <class SceneT>
class SoftShadowSystemGPU : public shs::AbstractSystem {
public:
    using Object = typename RenderTargetSystemGPU<SceneT>::Object;   // prev_model is not used

    SoftShadowSystemGPU(SceneT *scene, Device *dev, int shadow_size = 2048, int tile = 160)
        : scene_(scene), dev_(dev), sm_(shadow_size), tile_(tile) {}

    std::vector<Object> objects;

    void set_pcss(const shs_rt_pcss *pcss) { ok(shs_rt_set_pcss(dev_->ctx, pcss)); }   // nullptr: the demo's constants

    void process(float) override {
        shs::Canvas &canvas = *scene_->canvas;
        const int W = canvas.get_width(), H = canvas.get_height();
        const glm::mat4 view = scene_->viewer->camera->view_matrix, proj = scene_->viewer->camera->projection_matrix;
        std::vector<shs_rt_draw> draws(objects.size());
        for (size_t i = 0; i < objects.size(); ++i) {
            const Object &o = objects[i];
            shs_rt_draw &d = draws[i];
            d = shs_rt_draw{};
            d.mesh_id = o.mesh_id;
            d.albedo_tex = o.albedo_tex;
            const glm::mat4 mvp = proj * view * o.model;
            std::memcpy(d.model, glm::value_ptr(o.model), 64);
            std::memcpy(d.mvp, glm::value_ptr(mvp), 64);
            d.base_color[0] = o.base_color.r; d.base_color[1] = o.base_color.g; d.base_color[2] = o.base_color.b; d.base_color[3] = 255;
        }
        ok(shs_rt_render_shadow(dev_->ctx, sm_, sm_, tile_, tile_, glm::value_ptr(light_vp), draws.data(), (int32_t)draws.size()));
        shs_rt_frame f{};
        f.width = W; f.height = H; f.ref_tile_w = tile_; f.ref_tile_h = tile_;
        f.clear_color[0] = 20; f.clear_color[1] = 20; f.clear_color[2] = 25; f.clear_color[3] = 255;
        std::memcpy(f.view, glm::value_ptr(view), 64);
        std::memcpy(f.light_vp, glm::value_ptr(light_vp), 64);
        std::memcpy(f.light_dir_world, glm::value_ptr(light_dir_world), 12);
        std::memcpy(f.camera_pos, glm::value_ptr(scene_->viewer->position), 12);
        f.bias_base = 0.0025f; f.bias_slope = 0.01f;                                 // SHADOW_BIAS_BASE, SHADOW_BIAS_SLOPE
        f.flags = SHS_RT_USE_SHADOW;                                                 // (SHS_RT_PCF has no effect here)
        f.shading = 1;
        ok(shs_rt_render(dev_->ctx, &f, draws.data(), (int32_t)draws.size()));
        // shs_rt_resolve(ctx, colours, nullptr, nullptr) into the canvas, or shs_rt_device_targets for a device consumer
    }

    void ok(int rc) const {
        if (rc != SHS_OK) throw std::runtime_error(shs_last_error(dev_->ctx));
    }

    glm::mat4 light_vp{1.0f};
    glm::vec3 light_dir_world{0.4668f, -0.3487f, 0.8127f};   // LIGHT_DIR_WORLD :90 (the shader normalises it)

private:
    SceneT *scene_;
    Device *dev_;
    int sm_, tile_;
};

// -----------------------------------------------------------------------------------------------------
// Seam 1b, PBR -- hello-render-target/hello_pbr.cpp.
//
// Replaces RendererSystem::process there: PASS0 is the hard demo's (draw_triangle_tile_shadow :827-870), PASS1 the
// hard demo's raster (draw_triangle_tile_color_depth_motion :883-1045) with fragment_shader_pbr (:627-727) through
// shs_rt_render_pbr and shading = 2, PASS2 combined_motion_blur_pass (:1051-1252) through shs_canvas_motion_blur over
// shs_rt_device_targets.  The IBL precompute (:1855-1875) stays on the host at start-up; set_ibl hands its results
// over once.  skybox_background_pass (:733-799) is set_sky: the legacy AnalyticSky / CubeMapSky behind the triangles,
// bound per frame with the camera's vectors (shs_rt_set_sky does no device work); without it uncovered pixels keep the
// clear colour.  Uncompiled, like the other seams.
// -----------------------------------------------------------------------------------------------------
template <class SceneT>
class PbrSystemGPU : public shs::AbstractSystem {
public:
    struct Object {
        typename RenderTargetSystemGPU<SceneT>::Object geom;   // base_color is MaterialPBR::baseColor_srgb
        shs_rt_pbr_draw pbr;                                    // u.normal_mat, u.mat, the three IBL knobs (:474-518)
    };

    PbrSystemGPU(SceneT *scene, Device *dev, int shadow_size = 2048, int tile = 160)
        : scene_(scene), dev_(dev), sm_(shadow_size), tile_(tile) {}

    std::vector<Object> objects;     // geom.model / prev_model and pbr.normal_mat per frame

    void set_pbr(const shs_rt_pbr *k) { ok(shs_rt_set_pbr(dev_->ctx, k)); }   // nullptr: the demo's constants

    // EnvIBL (shs/resources/ibl.hpp:21-59) flattened to floats: the six faces of the irradiance map, then of each mip
    template <class EnvIblT>
    void set_ibl(const EnvIblT &ibl) {
        std::vector<float> irr, spec;
        auto put = [](std::vector<float> &out, const auto &cube) {
            for (int f = 0; f < 6; ++f)
                for (const glm::vec3 &c : cube.face[f]) { out.push_back(c.x); out.push_back(c.y); out.push_back(c.z); }
        };
        put(irr, ibl.env_irradiance);
        for (const auto &m : ibl.env_prefiltered_spec.mip) put(spec, m);
        ok(shs_rt_set_ibl(dev_->ctx, ibl.env_irradiance.size, irr.data(), ibl.env_prefiltered_spec.mip[0].size,
                          ibl.env_prefiltered_spec.mip_count(), spec.data()));
    }

    // skybox_background_pass (:733-799) of the demo's AnalyticSky through this frame's camera; call it before process().
    // A CubeMapSky host (hello_ibl_skybox.cpp:532-611) fills model = SHS_RT_SKY_CUBEMAP, encode = SHS_RT_SKY_ENCODE_CLAMP,
    // intensity and the six faces' shs_texture_upload ids instead.
    void set_sky(const glm::vec3 &sun_direction, float sky_exposure = 1.85f) {
        const shs::Camera3D &cam = *scene_->viewer->camera;
        shs_rt_sky s{};
        s.model = SHS_RT_SKY_ANALYTIC;
        s.encode = SHS_RT_SKY_ENCODE_REINHARD;
        std::memcpy(s.sun_dir, glm::value_ptr(sun_direction), 12);
        std::memcpy(s.cam_forward, glm::value_ptr(cam.direction_vector), 12);
        std::memcpy(s.cam_right, glm::value_ptr(cam.right_vector), 12);
        std::memcpy(s.cam_up, glm::value_ptr(cam.up_vector), 12);
        s.fov_degrees = cam.field_of_view;
        s.exposure = sky_exposure;
        ok(shs_rt_set_sky(dev_->ctx, &s));
    }
    void clear_sky() { ok(shs_rt_set_sky(dev_->ctx, nullptr)); }

    void process(float) override {
        shs::Canvas &canvas = *scene_->canvas;
        const int W = canvas.get_width(), H = canvas.get_height();
        const glm::mat4 view = scene_->viewer->camera->view_matrix, proj = scene_->viewer->camera->projection_matrix;
        std::vector<shs_rt_draw> draws(objects.size());
        std::vector<shs_rt_pbr_draw> mats(objects.size());
        for (size_t i = 0; i < objects.size(); ++i) {
            const auto &o = objects[i].geom;
            shs_rt_draw &d = draws[i];
            d.mesh_id = o.mesh_id;
            d.albedo_tex = o.albedo_tex;
            const glm::mat4 mvp = proj * view * o.model, prev_mvp = prev_vp_ * o.prev_model;
            std::memcpy(d.model, glm::value_ptr(o.model), 64);
            std::memcpy(d.mvp, glm::value_ptr(mvp), 64);
            std::memcpy(d.prev_mvp, glm::value_ptr(prev_mvp), 64);
            d.base_color[0] = o.base_color.r; d.base_color[1] = o.base_color.g; d.base_color[2] = o.base_color.b; d.base_color[3] = 255;
            mats[i] = objects[i].pbr;
        }
        ok(shs_rt_render_shadow(dev_->ctx, sm_, sm_, tile_, tile_, glm::value_ptr(light_vp), draws.data(), (int32_t)draws.size()));
        shs_rt_frame f{};
        f.width = W; f.height = H; f.ref_tile_w = tile_; f.ref_tile_h = tile_;
        f.clear_color[0] = 20; f.clear_color[1] = 20; f.clear_color[2] = 25; f.clear_color[3] = 255;
        std::memcpy(f.view, glm::value_ptr(view), 64);
        std::memcpy(f.light_vp, glm::value_ptr(light_vp), 64);
        std::memcpy(f.light_dir_world, glm::value_ptr(light_dir_world), 12);
        std::memcpy(f.camera_pos, glm::value_ptr(scene_->viewer->position), 12);
        f.bias_base = 0.0025f; f.bias_slope = 0.01f; f.max_velocity_px = 22.0f;      // SHADOW_BIAS_* :113-114, MB_MAX_PIXELS
        ok(render_pass1(f, draws.data(), mats.data(), (int32_t)draws.size()));
        void *color = nullptr, *depth = nullptr, *velocity = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &velocity));
        // PASS2 on the device (shs_canvas_motion_blur with SHS_CANVAS_DEVICE into a device buffer of the host's), or
        // shs_rt_resolve into rt->color / rt->depth / rt->velocity for a CPU PASS2.
        prev_vp_ = proj * view;
    }

    void ok(int rc) const {
        if (rc != SHS_OK) throw std::runtime_error(shs_last_error(dev_->ctx));
    }

    glm::mat4 light_vp{1.0f};
    glm::vec3 light_dir_world{0.4668f, -0.3487f, 0.8127f};   // LIGHT_DIR_WORLD (the shader normalises it)

protected:
    // PASS1's fragment shader: hello_pbr.cpp's under the 2x2 PCF.  PbrSoftShadowSystemGPU below replaces it.
    virtual int render_pass1(shs_rt_frame &f, const shs_rt_draw *draws, const shs_rt_pbr_draw *mats, int32_t n) {
        f.flags = SHS_RT_USE_SHADOW | SHS_RT_PCF;                                    // SHADOW_USE_PCF :117
        f.shading = 2;
        return shs_rt_render_pbr(dev_->ctx, &f, draws, mats, n);
    }

    SceneT *scene_;
    Device *dev_;

private:
    int sm_, tile_;
    glm::mat4 prev_vp_{1.0f};
};

// -----------------------------------------------------------------------------------------------------
// Seam 1b, PBR under PCSS -- hello-render-target/hello_pbr_light_shafts.cpp, PASS0 and PASS1.
//
// That demo's RendererSystem::process is hello_pbr.cpp's up to the fragment shader: PASS1 runs its own
// fragment_shader_pbr (:768-850) -- pcss_shadow_factor (:650-762) for the 2x2 PCF, no minimum ambient, a direct
// radiance of 3.0 -- through shs_rt_render_pbr_soft and shading = 3, over a 1024^2 map (SHADOW_MAP_SIZE :123) and tile
// jobs of 160.  The PCSS constants (:135-148) and the PBR constants are the context's defaults; set_pcss / set_pbr
// change them.  set_ibl and set_sky are PbrSystemGPU's.  LightShaftsGPU::apply (PASS1.5) and shs_canvas_motion_blur
// (PASS2) follow on the same stream.  Uncompiled, like the other seams.
// -----------------------------------------------------------------------------------------------------
template <class SceneT>
class PbrSoftShadowSystemGPU : public PbrSystemGPU<SceneT> {
public:
    PbrSoftShadowSystemGPU(SceneT *scene, Device *dev, int shadow_size = 1024, int tile = 160)
        : PbrSystemGPU<SceneT>(scene, dev, shadow_size, tile) {}

    void set_pcss(const shs_rt_pcss *pcss) { this->ok(shs_rt_set_pcss(this->dev_->ctx, pcss)); }   // nullptr: the demo's constants

protected:
    int render_pass1(shs_rt_frame &f, const shs_rt_draw *draws, const shs_rt_pbr_draw *mats, int32_t n) override {
        f.flags = SHS_RT_USE_SHADOW;                                                 // (SHS_RT_PCF has no effect here)
        f.shading = 3;
        return shs_rt_render_pbr_soft(this->dev_->ctx, &f, draws, mats, n);
    }
};

// -----------------------------------------------------------------------------------------------------
// Seam 1b, sky-lit -- hello-render-target/hello_ibl_skybox.cpp.
//
// Replaces RendererSystem::process there (:1106-1530), four calls on the context stream with no resolve in between:
//   1. shs_rt_render_shadow with tile jobs of 160 (TILE_SIZE_X / TILE_SIZE_Y :54-55): PASS0 (:646-686) is the hard demo's;
//   2. shs_rt_set_sky with SHS_RT_SKY_ENCODE_CLAMP and the viewer's camera: skybox_background_pass (:532-611), and the
//      same sky is u.sky of the camera pass (:1298) -- no device work, so it is bound per frame;
//   3. shs_rt_render_skybox_ibl, shading = 4: the hard demo's raster (:705-860) with this file's fragment_shader_full
//      (:446-524) and the per-object knobs (:1299-1302, :1362-1365, :1414-1417);
//   4. shs_canvas_motion_blur over shs_rt_device_targets into a device buffer of the host's: combined_motion_blur_pass
//      (:944-1060) is hello_pbr.cpp's (:1128-1252) operation for operation -- it forms glm::inverse(curr_vp) per pixel
//      where that one hoists it, and reads through accessors where that one reads raw pointers.
// The sky is the scene's CubeMapSky (six uploaded face textures, which cannot be released while bound) or its
// AnalyticSky; with neither bound the shader runs with u.sky == nullptr.  Uncompiled, like the other seams.
// -----------------------------------------------------------------------------------------------------
template <class SceneT>
class IblSkyboxSystemGPU : public shs::AbstractSystem {
public:
    struct Object {
        typename RenderTargetSystemGPU<SceneT>::Object geom;
        shs_rt_skybox_ibl_draw ibl{0.25f, 0.35f, 0.04f, 1.0f};   // Uniforms :336-339
    };

    IblSkyboxSystemGPU(SceneT *scene, Device *dev, void *blurred_dev, int shadow_size = 2048, int tile = 160)
        : scene_(scene), dev_(dev), blurred_(blurred_dev), sm_(shadow_size), tile_(tile) {}

    std::vector<Object> objects;     // geom.model / prev_model per frame

    // The scene's sky: a CubeMapSky's faces (+X -X +Y -Y +Z -Z, shs_texture_upload ids) and intensity_, or an
    // AnalyticSky's sun_direction.  The camera's vectors are filled in by process().
    void use_cubemap(const int32_t face_tex[6], float intensity) {
        sky_ = shs_rt_sky{};
        sky_.model = SHS_RT_SKY_CUBEMAP;
        std::memcpy(sky_.face_tex, face_tex, sizeof sky_.face_tex);
        sky_.intensity = intensity;
    }
    void use_analytic(const glm::vec3 &sun_direction) {
        sky_ = shs_rt_sky{};
        sky_.model = SHS_RT_SKY_ANALYTIC;
        std::memcpy(sky_.sun_dir, glm::value_ptr(sun_direction), 12);
    }
    void use_no_sky() { sky_ = shs_rt_sky{}; }

    void process(float) override {
        shs::Canvas &canvas = *scene_->canvas;
        const int W = canvas.get_width(), H = canvas.get_height();
        const shs::Camera3D &cam = *scene_->viewer->camera;
        const glm::mat4 view = cam.view_matrix, proj = cam.projection_matrix;
        std::vector<shs_rt_draw> draws(objects.size());
        std::vector<shs_rt_skybox_ibl_draw> knobs(objects.size());
        for (size_t i = 0; i < objects.size(); ++i) {
            const auto &o = objects[i].geom;
            shs_rt_draw &d = draws[i];
            d.mesh_id = o.mesh_id;
            d.albedo_tex = o.albedo_tex;
            const glm::mat4 mvp = proj * view * o.model, prev_mvp = prev_proj_ * prev_view_ * o.prev_model;
            std::memcpy(d.model, glm::value_ptr(o.model), 64);
            std::memcpy(d.mvp, glm::value_ptr(mvp), 64);
            std::memcpy(d.prev_mvp, glm::value_ptr(prev_mvp), 64);
            d.base_color[0] = o.base_color.r; d.base_color[1] = o.base_color.g; d.base_color[2] = o.base_color.b; d.base_color[3] = 255;
            knobs[i] = objects[i].ibl;
        }
        // 1. PASS0
        ok(shs_rt_render_shadow(dev_->ctx, sm_, sm_, tile_, tile_, glm::value_ptr(light_vp), draws.data(), (int32_t)draws.size()));
        // 2. the sky through this frame's camera, for the camera pass's shader and the background behind it
        if (sky_.model != SHS_RT_SKY_NONE) {
            sky_.encode = SHS_RT_SKY_ENCODE_CLAMP;                                   // :598-601
            std::memcpy(sky_.cam_forward, glm::value_ptr(cam.direction_vector), 12);
            std::memcpy(sky_.cam_right, glm::value_ptr(cam.right_vector), 12);
            std::memcpy(sky_.cam_up, glm::value_ptr(cam.up_vector), 12);
            sky_.fov_degrees = cam.field_of_view;
            ok(shs_rt_set_sky(dev_->ctx, &sky_));
        } else {
            ok(shs_rt_set_sky(dev_->ctx, nullptr));
        }
        // 3. PASS1
        shs_rt_frame f{};
        f.width = W; f.height = H; f.ref_tile_w = tile_; f.ref_tile_h = tile_;
        f.clear_color[0] = 20; f.clear_color[1] = 20; f.clear_color[2] = 25; f.clear_color[3] = 255;
        std::memcpy(f.view, glm::value_ptr(view), 64);
        std::memcpy(f.light_vp, glm::value_ptr(light_vp), 64);
        std::memcpy(f.light_dir_world, glm::value_ptr(light_dir_world), 12);
        std::memcpy(f.camera_pos, glm::value_ptr(scene_->viewer->position), 12);
        f.bias_base = 0.0025f; f.bias_slope = 0.01f; f.max_velocity_px = 22.0f;      // SHADOW_BIAS_*, MB_MAX_PIXELS :76
        f.flags = SHS_RT_USE_SHADOW | SHS_RT_PCF;
        f.shading = 4;
        ok(shs_rt_render_skybox_ibl(dev_->ctx, &f, draws.data(), knobs.data(), (int32_t)draws.size()));
        // 4. PASS2 over the planes the camera pass left on the device (MB_* :74-82)
        void *color = nullptr, *depth = nullptr, *velocity = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &velocity));
        shs_canvas_motion_blur_desc mb{};
        mb.width = W; mb.height = H;
        std::memcpy(mb.curr_view, glm::value_ptr(view), 64);
        std::memcpy(mb.curr_proj, glm::value_ptr(proj), 64);
        std::memcpy(mb.prev_view, glm::value_ptr(prev_view_), 64);
        std::memcpy(mb.prev_proj, glm::value_ptr(prev_proj_), 64);
        mb.samples = 12; mb.strength = 0.85f; mb.w_obj = 1.0f; mb.w_cam = 0.35f; mb.soft_knee = 1; mb.knee_px = 18.0f; mb.max_px = 22.0f;
        ok(shs_canvas_motion_blur(dev_->ctx, &mb, static_cast<const uint8_t *>(color), static_cast<const float *>(depth),
                                  static_cast<const float *>(velocity), static_cast<uint8_t *>(blurred_), SHS_CANVAS_DEVICE));
        prev_view_ = view;
        prev_proj_ = proj;
    }

    void ok(int rc) const {
        if (rc != SHS_OK) throw std::runtime_error(shs_last_error(dev_->ctx));
    }

    glm::mat4 light_vp{1.0f};
    glm::vec3 light_dir_world{0.4668f, -0.3487f, 0.8127f};   // (the shader normalises it)

private:
    SceneT *scene_;
    Device *dev_;
    void *blurred_;                  // W * H Color on the device: the frame the host presents
    int sm_, tile_;
    shs_rt_sky sky_{};
    glm::mat4 prev_view_{1.0f}, prev_proj_{1.0f};
};

// -----------------------------------------------------------------------------------------------------
// Seam 1b, IBL-lit -- hello-render-target/hello_ibl_skybox_optimized.cpp and hello_ibl_skybox_xsimd.cpp.
//
// Replaces RendererSystem::process of either file (optimized :1572-1970), four calls on the context stream with no
// resolve in between:
//   1. PASS0 with tile jobs of 160 over the 2048^2 map (TILE_SIZE_X / TILE_SIZE_Y :127-128, SHADOW_MAP_SIZE :133):
//      shs_rt_render_shadow for the optimized file (its draw_triangle_tile_shadow :1065-1108 is the hard demo's), or
//      shs_rt_render_shadow_edge for the xsimd file (draw_triangle_tile_shadow_xsimd, xsimd :1016-1191), whose simd_lanes
//      is xsimd::batch<float>::size of the build being replaced (8 for AVX2, 4 for SSE2 / NEON, 16 for AVX-512);
//   2. shs_rt_set_sky with SHS_RT_SKY_CUBEMAP, SHS_RT_SKY_ENCODE_CLAMP and the viewer's camera: skybox_background_pass;
//   3. shs_rt_render_ibl_phong, shading = 11: the hard demo's raster (:1125-1291) with these files' fragment_shader_full
//      (:875-958) and the per-object knobs (:1737-1741, :1805-1809, :1862-1866), over the IBL bound once by set_ibl()
//      below -- the host's own precompute (build_irradiance_cubemap, build_prefiltered_spec) through shs_rt_set_ibl;
//   4. shs_canvas_motion_blur over shs_rt_device_targets into a device buffer of the host's, with MB_* :147-155
//      (combined_motion_blur_pass of both files is that pass: DESIGN.md section 4).
// Uncompiled, like the other seams.
// -----------------------------------------------------------------------------------------------------
template <class SceneT>
class IblPhongSystemGPU : public shs::AbstractSystem {
public:
    struct Object {
        typename RenderTargetSystemGPU<SceneT>::Object geom;
        shs_rt_ibl_phong_draw ibl{0.30f, 0.35f, 0.04f, 1.0f, 64.0f};   // Uniforms :757-764
    };

    // simd_lanes 0: the optimized file's PASS0; else the xsimd file's, with that batch size
    IblPhongSystemGPU(SceneT *scene, Device *dev, void *blurred_dev, int simd_lanes = 0, int shadow_size = 2048, int tile = 160)
        : scene_(scene), dev_(dev), blurred_(blurred_dev), lanes_(simd_lanes), sm_(shadow_size), tile_(tile) {}

    std::vector<Object> objects;     // geom.model / prev_model per frame

    // IBLResources (:520-527) once after the host's precompute: irradiance.face[f] and spec.mip[m].face[f] as rgb floats,
    // the six faces of a level one after the other, the mips concatenated (mip m of size max(1, base >> m))
    void set_ibl(int irr_size, const float *irr, int spec_base, int mip_count, const float *spec) {
        ok(shs_rt_set_ibl(dev_->ctx, irr_size, irr, spec_base, mip_count, spec));
    }
    void use_cubemap(const int32_t face_tex[6], float intensity) {
        sky_ = shs_rt_sky{};
        sky_.model = SHS_RT_SKY_CUBEMAP;
        std::memcpy(sky_.face_tex, face_tex, sizeof sky_.face_tex);
        sky_.intensity = intensity;
    }

    void process(float) override {
        shs::Canvas &canvas = *scene_->canvas;
        const int W = canvas.get_width(), H = canvas.get_height();
        const shs::Camera3D &cam = *scene_->viewer->camera;
        const glm::mat4 view = cam.view_matrix, proj = cam.projection_matrix;
        std::vector<shs_rt_draw> draws(objects.size());
        std::vector<shs_rt_ibl_phong_draw> knobs(objects.size());
        for (size_t i = 0; i < objects.size(); ++i) {
            const auto &o = objects[i].geom;
            shs_rt_draw &d = draws[i];
            d.mesh_id = o.mesh_id;
            d.albedo_tex = o.albedo_tex;
            const glm::mat4 mvp = proj * view * o.model, prev_mvp = prev_proj_ * prev_view_ * o.prev_model;
            std::memcpy(d.model, glm::value_ptr(o.model), 64);
            std::memcpy(d.mvp, glm::value_ptr(mvp), 64);
            std::memcpy(d.prev_mvp, glm::value_ptr(prev_mvp), 64);
            d.base_color[0] = o.base_color.r; d.base_color[1] = o.base_color.g; d.base_color[2] = o.base_color.b; d.base_color[3] = 255;
            knobs[i] = objects[i].ibl;
        }
        // 1. PASS0
        if (lanes_ > 0)
            ok(shs_rt_render_shadow_edge(dev_->ctx, sm_, sm_, tile_, tile_, glm::value_ptr(light_vp), draws.data(), (int32_t)draws.size(), lanes_));
        else
            ok(shs_rt_render_shadow(dev_->ctx, sm_, sm_, tile_, tile_, glm::value_ptr(light_vp), draws.data(), (int32_t)draws.size()));
        // 2. the sky through this frame's camera, for the background behind the camera pass
        if (sky_.model != SHS_RT_SKY_NONE) {
            sky_.encode = SHS_RT_SKY_ENCODE_CLAMP;
            std::memcpy(sky_.cam_forward, glm::value_ptr(cam.direction_vector), 12);
            std::memcpy(sky_.cam_right, glm::value_ptr(cam.right_vector), 12);
            std::memcpy(sky_.cam_up, glm::value_ptr(cam.up_vector), 12);
            sky_.fov_degrees = cam.field_of_view;
            ok(shs_rt_set_sky(dev_->ctx, &sky_));
        } else {
            ok(shs_rt_set_sky(dev_->ctx, nullptr));
        }
        // 3. PASS1
        shs_rt_frame f{};
        f.width = W; f.height = H; f.ref_tile_w = tile_; f.ref_tile_h = tile_;
        f.clear_color[0] = 20; f.clear_color[1] = 20; f.clear_color[2] = 25; f.clear_color[3] = 255;
        std::memcpy(f.view, glm::value_ptr(view), 64);
        std::memcpy(f.light_vp, glm::value_ptr(light_vp), 64);
        std::memcpy(f.light_dir_world, glm::value_ptr(light_dir_world), 12);
        std::memcpy(f.camera_pos, glm::value_ptr(scene_->viewer->position), 12);
        f.bias_base = 0.0025f; f.bias_slope = 0.01f; f.max_velocity_px = 22.0f;      // SHADOW_BIAS_* :138-139, MB_MAX_PIXELS :149
        f.flags = SHS_RT_USE_SHADOW | SHS_RT_PCF;
        f.shading = 11;
        ok(shs_rt_render_ibl_phong(dev_->ctx, &f, draws.data(), knobs.data(), (int32_t)draws.size()));
        // 4. PASS2 over the planes the camera pass left on the device (MB_* :147-155)
        void *color = nullptr, *depth = nullptr, *velocity = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &velocity));
        shs_canvas_motion_blur_desc mb{};
        mb.width = W; mb.height = H;
        std::memcpy(mb.curr_view, glm::value_ptr(view), 64);
        std::memcpy(mb.curr_proj, glm::value_ptr(proj), 64);
        std::memcpy(mb.prev_view, glm::value_ptr(prev_view_), 64);
        std::memcpy(mb.prev_proj, glm::value_ptr(prev_proj_), 64);
        mb.samples = 12; mb.strength = 0.85f; mb.w_obj = 1.0f; mb.w_cam = 0.35f; mb.soft_knee = 1; mb.knee_px = 18.0f; mb.max_px = 22.0f;
        ok(shs_canvas_motion_blur(dev_->ctx, &mb, static_cast<const uint8_t *>(color), static_cast<const float *>(depth),
                                  static_cast<const float *>(velocity), static_cast<uint8_t *>(blurred_), SHS_CANVAS_DEVICE));
        prev_view_ = view;
        prev_proj_ = proj;
    }

    void ok(int rc) const {
        if (rc != SHS_OK) throw std::runtime_error(shs_last_error(dev_->ctx));
    }

    glm::mat4 light_vp{1.0f};
    glm::vec3 light_dir_world{0.4668f, -0.3487f, 0.8127f};   // (the shader normalises it)

private:
    SceneT *scene_;
    Device *dev_;
    void *blurred_;                  // W * H Color on the device: the frame the host presents
    int lanes_, sm_, tile_;
    shs_rt_sky sky_{};
    glm::mat4 prev_view_{1.0f}, prev_proj_{1.0f};
};

// -----------------------------------------------------------------------------------------------------
// Seam 1b, water -- hello-render-target/hello_water.cpp.
//
// Replaces RendererSystem::process there, five calls on the context stream with no resolve in between:
//   1. shs_rt_render_shadow with tile jobs of 80: PASS0 is the hard demo's;
//   2. shs_rt_render_water, shading = 5, from the camera mirrored at y = WATER_Y (compute_reflection_view_lh :1550-1563,
//      formed here on the host): PASS1A (:1765-1955), the objects alone, every draw non-water, no reflection bound, the
//      mirrored position as camera_pos (:1804);
//   3. shs_rt_keep_reflection: that pass's colour plane becomes u.reflection_color (one device-to-device copy);
//   4. shs_rt_render_water again through the viewer's camera with the floor, the water plane (SHS_RT_WATER_SURFACE) and
//      the objects, SHS_RT_WATER_REFLECTION and reflection_vp = proj * refl_view: PASS1B (:1957-2211);
//   5. shs_canvas_motion_blur over shs_rt_device_targets: combined_motion_blur_pass is the hard demo's text.
// The demo binds no sky: uncovered pixels keep CLEAR_BG (:86).  Uncompiled, like the other seams.
// -----------------------------------------------------------------------------------------------------
template <class SceneT>
class WaterSystemGPU : public shs::AbstractSystem {
public:
    struct Object {
        typename RenderTargetSystemGPU<SceneT>::Object geom;
        bool water = false;          // the water plane: fragment_shader_water; it is left out of the reflection pass
    };

    WaterSystemGPU(SceneT *scene, Device *dev, void *blurred_dev, float water_y = -0.20f, int shadow_size = 2048, int tile = 80)
        : scene_(scene), dev_(dev), blurred_(blurred_dev), water_y_(water_y), sm_(shadow_size), tile_(tile) {}

    std::vector<Object> objects;     // geom.model / prev_model per frame

    void process(float dt) override {
        time_accum_ += dt;
        shs::Canvas &canvas = *scene_->canvas;
        const int W = canvas.get_width(), H = canvas.get_height();
        const shs::Camera3D &cam = *scene_->viewer->camera;
        const glm::mat4 view = cam.view_matrix, proj = cam.projection_matrix;
        // compute_reflection_view_lh :1550-1563
        glm::vec3 rpos = scene_->viewer->position, rdir = cam.direction_vector, rup = cam.up_vector;
        rpos.y = 2.0f * water_y_ - rpos.y;
        rdir.y = -rdir.y;
        rup.y = -rup.y;
        const glm::mat4 refl_view = glm::lookAtLH(rpos, rpos + rdir, rup);
        const glm::mat4 refl_vp = proj * refl_view;
        std::vector<shs_rt_draw> draws(objects.size()), refl_draws;
        std::vector<shs_rt_water_draw> flags(objects.size()), refl_flags;
        for (size_t i = 0; i < objects.size(); ++i) {
            const auto &o = objects[i].geom;
            shs_rt_draw &d = draws[i];
            d.mesh_id = o.mesh_id;
            d.albedo_tex = o.albedo_tex;
            const glm::mat4 mvp = proj * view * o.model, prev_mvp = prev_proj_ * prev_view_ * o.prev_model;
            std::memcpy(d.model, glm::value_ptr(o.model), 64);
            std::memcpy(d.mvp, glm::value_ptr(mvp), 64);
            std::memcpy(d.prev_mvp, glm::value_ptr(prev_mvp), 64);
            d.base_color[0] = o.base_color.r; d.base_color[1] = o.base_color.g; d.base_color[2] = o.base_color.b; d.base_color[3] = 255;
            flags[i].flags = objects[i].water ? SHS_RT_WATER_SURFACE : 0u;
            if (!objects[i].water) {
                shs_rt_draw r = d;
                const glm::mat4 rmvp = refl_vp * o.model;
                std::memcpy(r.mvp, glm::value_ptr(rmvp), 64);
                std::memcpy(r.prev_mvp, glm::value_ptr(rmvp), 64);
                refl_draws.push_back(r);
                refl_flags.push_back(shs_rt_water_draw{0u});
            }
        }
        // 1. PASS0
        ok(shs_rt_render_shadow(dev_->ctx, sm_, sm_, tile_, tile_, glm::value_ptr(light_vp), draws.data(), (int32_t)draws.size()));
        shs_rt_frame f{};
        f.width = W; f.height = H; f.ref_tile_w = tile_; f.ref_tile_h = tile_;
        f.clear_color[0] = 24; f.clear_color[1] = 34; f.clear_color[2] = 58; f.clear_color[3] = 255;   // CLEAR_BG :86
        std::memcpy(f.light_vp, glm::value_ptr(light_vp), 64);
        std::memcpy(f.light_dir_world, glm::value_ptr(light_dir_world), 12);
        f.bias_base = 0.0025f; f.bias_slope = 0.01f; f.max_velocity_px = 22.0f;      // SHADOW_BIAS_*, MB_MAX_PIXELS
        f.flags = SHS_RT_USE_SHADOW | SHS_RT_PCF;
        f.shading = 5;
        shs_rt_water wu{};
        wu.time_sec = time_accum_;
        // 2. PASS1A from the mirrored camera, 3. keep its colour
        shs_rt_frame rf = f;
        std::memcpy(rf.view, glm::value_ptr(refl_view), 64);
        std::memcpy(rf.camera_pos, glm::value_ptr(rpos), 12);
        std::memcpy(wu.reflection_vp, glm::value_ptr(glm::mat4(1.0f)), 64);
        wu.flags = 0u;
        ok(shs_rt_render_water(dev_->ctx, &rf, refl_draws.data(), refl_flags.data(), &wu, (int32_t)refl_draws.size()));
        ok(shs_rt_keep_reflection(dev_->ctx));
        // 4. PASS1B
        std::memcpy(f.view, glm::value_ptr(view), 64);
        std::memcpy(f.camera_pos, glm::value_ptr(scene_->viewer->position), 12);
        std::memcpy(wu.reflection_vp, glm::value_ptr(refl_vp), 64);
        wu.flags = SHS_RT_WATER_REFLECTION;
        ok(shs_rt_render_water(dev_->ctx, &f, draws.data(), flags.data(), &wu, (int32_t)draws.size()));
        // 5. PASS2 over the planes the camera pass left on the device (MB_*)
        void *color = nullptr, *depth = nullptr, *velocity = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &velocity));
        shs_canvas_motion_blur_desc mb{};
        mb.width = W; mb.height = H;
        std::memcpy(mb.curr_view, glm::value_ptr(view), 64);
        std::memcpy(mb.curr_proj, glm::value_ptr(proj), 64);
        std::memcpy(mb.prev_view, glm::value_ptr(prev_view_), 64);
        std::memcpy(mb.prev_proj, glm::value_ptr(prev_proj_), 64);
        mb.samples = 12; mb.strength = 0.85f; mb.w_obj = 1.0f; mb.w_cam = 0.35f; mb.soft_knee = 1; mb.knee_px = 18.0f; mb.max_px = 22.0f;
        ok(shs_canvas_motion_blur(dev_->ctx, &mb, static_cast<const uint8_t *>(color), static_cast<const float *>(depth),
                                  static_cast<const float *>(velocity), static_cast<uint8_t *>(blurred_), SHS_CANVAS_DEVICE));
        prev_view_ = view;
        prev_proj_ = proj;
    }

    void ok(int rc) const {
        if (rc != SHS_OK) throw std::runtime_error(shs_last_error(dev_->ctx));
    }

    glm::mat4 light_vp{1.0f};
    glm::vec3 light_dir_world{0.4668f, -0.3487f, 0.8127f};   // (the shaders normalise it)

private:
    SceneT *scene_;
    Device *dev_;
    void *blurred_;                  // W * H Color on the device: the frame the host presents
    float water_y_, time_accum_ = 0.0f;
    int sm_, tile_;
    glm::mat4 prev_view_{1.0f}, prev_proj_{1.0f};
};

// -----------------------------------------------------------------------------------------------------
// Seam 1c, light shafts -- hello-render-target/hello_pbr_light_shafts.cpp, PASS1.5.
//
// light_shafts_pass (:1525-1707) as RendererSystem::process calls it (:2171-2190), over the planes the camera pass
// left on the device: after a PbrSystemGPU::process (or any shs_rt_render*) call apply(); the colour plane of
// shs_rt_device_targets is rewritten in place, the shadow map is the one of shs_rt_device_shadow_map, and
// shs_canvas_motion_blur (PASS2) follows on the same stream.  ParamsT is that file's LightShaftParams (:189-218).
// That demo's PASS1 shader is not hello_pbr.cpp's (PCSS instead of the 2x2 PCF, no minimum ambient): it is
// PbrSoftShadowSystemGPU above, not PbrSystemGPU.  Uncompiled, like the other seams.
// -----------------------------------------------------------------------------------------------------
template <class SceneT>
class LightShaftsGPU {
public:
    LightShaftsGPU(SceneT *scene, Device *dev) : scene_(scene), dev_(dev) {}

    template <class ParamsT>
    void apply(const ParamsT &p, const glm::vec3 &sun_dir_world, const glm::mat4 &light_vp) {
        shs::Canvas &canvas = *scene_->canvas;
        const glm::mat4 inv_vp = glm::inverse(scene_->viewer->camera->projection_matrix * scene_->viewer->camera->view_matrix);
        shs_canvas_light_shafts_desc d{};
        d.width = canvas.get_width();
        d.height = canvas.get_height();
        std::memcpy(d.cam_pos, glm::value_ptr(scene_->viewer->position), 12);
        std::memcpy(d.inv_view_proj, glm::value_ptr(inv_vp), 64);
        std::memcpy(d.sun_dir_world, glm::value_ptr(sun_dir_world), 12);
        std::memcpy(d.light_vp, glm::value_ptr(light_vp), 64);
        d.enable = p.enable; d.steps = p.steps; d.max_dist = p.max_dist; d.min_dist = p.min_dist;
        d.base_density = p.base_density; d.height_falloff = p.height_falloff;
        d.noise_scale = p.noise_scale; d.noise_strength = p.noise_strength; d.jitter_amount = p.jitter_amount;
        d.ambient_strength = p.ambient_strength; d.sigma_s = p.sigma_s; d.sigma_t = p.sigma_t; d.g = p.g;
        d.intensity = p.intensity; d.use_shadow = p.use_shadow; d.shadow_bias = p.shadow_bias; d.shadow_pcf_2x2 = p.shadow_pcf_2x2;
        void *color = nullptr, *depth = nullptr, *map = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, nullptr));
        if (shs_rt_device_shadow_map(dev_->ctx, &map, &d.shadow_w, &d.shadow_h) != SHS_OK) map = nullptr;   // no PASS0: all lit
        ok(shs_canvas_light_shafts(dev_->ctx, &d, static_cast<const uint8_t *>(color), static_cast<const float *>(depth),
                                   static_cast<const float *>(map), static_cast<uint8_t *>(color), nullptr, SHS_CANVAS_DEVICE));
    }

    void ok(int rc) const {
        if (rc != SHS_OK) throw std::runtime_error(shs_last_error(dev_->ctx));
    }

private:
    SceneT *scene_;
    Device *dev_;
};

// -----------------------------------------------------------------------------------------------------
// Seam 1c, post chains -- hello-render-target/hello_multi_pass.cpp (:1379-1426),
// hello_camera_and_perobject_motion_blur.cpp (:1544-1606) and hello_glowing_star.cpp (:1233-1310).
//
// Everything those main loops do between sys->render() and copy_to_SDLSurface, as one call over the planes the
// raster left on the device (shs_rt_device_targets), or over the demo's own RT_ColorDepthMotion when the raster ran
// on the host.  The defaults are the demos' file-scope constants; a host with other values sets the desc's members.
// present(): the frame into the canvas the demo presents (fxaa_out / final_out), the only copy back.  Uncompiled,
// like the other seams.
// -----------------------------------------------------------------------------------------------------
class PostChainGPU {
public:
    explicit PostChainGPU(Device *dev) : dev_(dev) {}

    // hello_multi_pass.cpp's constants (:66-100)
    static shs_canvas_multi_pass_frame_desc multi_pass_defaults(int W, int H) {
        shs_canvas_multi_pass_frame_desc d{};
        d.width = W; d.height = H;
        d.blur_mode = SHS_CANVAS_BLUR_VELOCITY_FIRST;
        d.enable_dof = 1; d.enable_fxaa = 1;
        d.velocity_blur.samples = 12; d.velocity_blur.strength = 1.0f;
        d.dof.blur_iterations = 4; d.dof.autofocus_radius = 6; d.dof.focus_x = W / 2; d.dof.focus_y = H / 2;
        d.dof.range = 34.0f; d.dof.max_blur = 0.75f;
        const uint8_t fog[4] = {28, 30, 38, 255};
        std::memcpy(d.fog.fog_color, fog, 4);
        d.fog.fog_start = 20.0f; d.fog.fog_end = 80.0f; d.fog.fog_power = 1.25f;
        d.outline.radius = 1; d.outline.threshold = 0.75f; d.outline.strength = 0.15f;
        d.fxaa.reduce_min = 1.0f / 128.0f; d.fxaa.reduce_mul = 1.0f / 8.0f; d.fxaa.span_max = 8.0f;
        return d;
    }

    // hello_camera_and_perobject_motion_blur.cpp: the same passes in its order, combined_motion_blur_pass after the
    // outline.  The caller fills the motion blur's constants (MB_*) once; the matrices change every frame.
    static void use_combined_blur(shs_canvas_multi_pass_frame_desc &d, const glm::mat4 &curr_view, const glm::mat4 &curr_proj,
                                  const glm::mat4 &prev_view, const glm::mat4 &prev_proj) {
        d.blur_mode = SHS_CANVAS_BLUR_COMBINED_LATE;
        std::memcpy(d.motion_blur.curr_view, glm::value_ptr(curr_view), 64);
        std::memcpy(d.motion_blur.curr_proj, glm::value_ptr(curr_proj), 64);
        std::memcpy(d.motion_blur.prev_view, glm::value_ptr(prev_view), 64);
        std::memcpy(d.motion_blur.prev_proj, glm::value_ptr(prev_proj), 64);
    }

    // hello_glowing_star.cpp's constants (:62-90)
    static shs_canvas_glow_frame_desc glow_defaults(int W, int H) {
        shs_canvas_glow_frame_desc d{};
        d.width = W; d.height = H;
        d.enable_dof = 1; d.enable_bloom = 1; d.enable_flare = 1; d.bloom_iterations = 10;
        d.velocity_blur.samples = 8; d.velocity_blur.strength = 1.5f;
        d.dof.blur_iterations = 3; d.dof.autofocus_radius = 6; d.dof.focus_x = W / 2; d.dof.focus_y = H / 2;
        d.dof.range = 22.0f; d.dof.max_blur = 0.80f;
        d.spec_bright.threshold = 0.139f; d.spec_bright.intensity = 13.25f;
        d.lens_flare.intensity = 0.55f; d.lens_flare.halo_intensity = 0.35f; d.lens_flare.chroma_shift_px = 0.8f;
        d.lens_flare.n_ghosts = 3;
        const float scales[3] = {0.55f, 0.85f, 1.25f};
        std::memcpy(d.lens_flare.ghost_scales, scales, sizeof scales);
        return d;
    }

    // over the last shs_rt_render*'s planes; frame: a device buffer of the host's, W*H*4 bytes
    void multi_pass(const shs_canvas_multi_pass_frame_desc &d, void *frame) {
        void *color = nullptr, *depth = nullptr, *vel = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &vel));
        ok(shs_canvas_multi_pass_frame(dev_->ctx, &d, static_cast<const uint8_t *>(color), static_cast<const float *>(depth),
                                       static_cast<const float *>(vel), static_cast<uint8_t *>(frame), SHS_CANVAS_DEVICE));
    }

    // the star's chain over the last shs_rt_render_motion's planes (shading 7: the spec plane comes with them)
    void glow(const shs_canvas_glow_frame_desc &d, void *frame) {
        void *color = nullptr, *depth = nullptr, *vel = nullptr, *spec = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &vel));
        ok(shs_rt_device_spec(dev_->ctx, &spec));
        ok(shs_canvas_glow_frame(dev_->ctx, &d, static_cast<const uint8_t *>(color), static_cast<const float *>(depth),
                                 static_cast<const float *>(vel), static_cast<const float *>(spec), static_cast<uint8_t *>(frame),
                                 SHS_CANVAS_DEVICE));
    }

    // hello_per_object_motion_blur.cpp:786 over the last shs_rt_render_plain's planes (shading 8).  That pass leaves the
    // depth plane in SCREEN rows, as the demo's ZBuffer holds it: depth_rows = 1.  velocity_scale: the host's
    // clampf(target_dt / dt, 0.25f, 4.0f) (:782-784).  frame: a device buffer of the host's, W*H*4 bytes, not the colour plane.
    static shs_canvas_object_blur_desc object_blur_defaults(int W, int H, float velocity_scale) {
        shs_canvas_object_blur_desc d{};
        d.width = W; d.height = H;
        d.multiplier = 1.85f; d.velocity_scale = velocity_scale; d.min_vel2 = 0.25f; d.max_samples = 20; d.depth_eps = 0.15f;
        d.depth_rows = 1;
        return d;
    }
    void object_blur(const shs_canvas_object_blur_desc &d, void *frame) {
        void *color = nullptr, *depth = nullptr, *vel = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &vel));
        ok(shs_canvas_object_blur(dev_->ctx, &d, static_cast<const uint8_t *>(color), static_cast<const float *>(depth),
                                  static_cast<const float *>(vel), static_cast<uint8_t *>(frame), SHS_CANVAS_DEVICE));
    }

    // hello_depth_of_field.cpp:786-812 over the last shs_rt_render_plain's planes (shading 9), in place on the colour plane.
    // The depth plane goes in as it lies, in screen rows: that demo reads its ZBuffer unflipped (:270, :321).
    static shs_canvas_dof_desc dof_defaults(int W, int H) {
        shs_canvas_dof_desc d{};
        d.width = W; d.height = H;
        d.blur_iterations = 3; d.autofocus_radius = 6; d.focus_x = W / 2; d.focus_y = H / 2;
        d.range = 24.0f; d.max_blur = 0.6f;
        return d;
    }
    void dof(const shs_canvas_dof_desc &d) {
        void *color = nullptr, *depth = nullptr, *vel = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &vel));
        ok(shs_canvas_dof(dev_->ctx, &d, static_cast<uint8_t *>(color), static_cast<const float *>(depth), nullptr, nullptr, SHS_CANVAS_DEVICE));
    }

    // hello_ping_pong.cpp:611-618 over the last shs_rt_render_plain's colour plane (shading 10), in place
    void ping_pong(int W, int H, int iterations = 3) {
        void *color = nullptr, *depth = nullptr, *vel = nullptr;
        ok(shs_rt_device_targets(dev_->ctx, &color, &depth, &vel));
        ok(shs_canvas_ping_pong_blur(dev_->ctx, W, H, iterations, static_cast<uint8_t *>(color), SHS_CANVAS_DEVICE));
    }

    // the demo's own targets on the host (RT_ColorDepthMotion: color, depth, motion) into the canvas it presents
    template <class RtT>
    void multi_pass_host(const shs_canvas_multi_pass_frame_desc &d, RtT &rt, shs::Canvas &fxaa_out) {
        ok(shs_canvas_multi_pass_frame(dev_->ctx, &d, reinterpret_cast<const uint8_t *>(rt.color.buffer().raw()),
                                       rt.depth.buffer().raw(), &rt.motion.vel[0].x,   // MotionBuffer::vel (:453-489)
                                       reinterpret_cast<uint8_t *>(fxaa_out.buffer().raw()), 0));
    }

    // hello_glowing_star.cpp's RT (color, depth, velocity, spec) into final_out
    template <class RtT>
    void glow_host(const shs_canvas_glow_frame_desc &d, RtT &rt, shs::Canvas &final_out) {
        ok(shs_canvas_glow_frame(dev_->ctx, &d, reinterpret_cast<const uint8_t *>(rt.color.buffer().raw()),
                                 rt.depth.buffer().raw(), &rt.velocity.raw()[0].x, rt.spec.raw(),
                                 reinterpret_cast<uint8_t *>(final_out.buffer().raw()), 0));
    }

    void ok(int rc) const {
        if (rc != SHS_OK) throw std::runtime_error(shs_last_error(dev_->ctx));
    }

private:
    Device *dev_;
};

// -----------------------------------------------------------------------------------------------------
// Seam 1c, the raster of those three demos -- RendererSystem::process of hello_multi_pass.cpp,
// hello_camera_and_perobject_motion_blur.cpp and hello_glowing_star.cpp.
//
// Their tile jobs over draw_triangle_tile_color_depth_motion (hello_multi_pass.cpp:525-599) / the star's single call of
// draw_triangle_color_depth_velocity_spec (hello_glowing_star.cpp:354-435) become one shs_rt_render_motion; the whole
// frame is then
//   raster.process(dt);                       // colour, depth, velocity (and spec) stay on the device
//   chain.multi_pass(desc, frame_dev);        // hello_multi_pass.cpp; with use_combined_blur(desc, ...) the other blur demo
//   chain.glow(glow_desc, frame_dev);         // hello_glowing_star.cpp
// and one copy of frame_dev into the canvas the demo presents.  star: shading 7 and a single job covering the frame;
// otherwise shading 6 and tile jobs of `tile`.  max_velocity_px: MB_MAX_PIXELS, 40 / 22 / 30 in the three demos.
// Objects are RenderTargetSystemGPU's (mesh_id, model, prev_model, base_color); a texture is rejected.
//
// The three plain demos are the same raster through shs_rt_render_plain: set plain_shading to 8
// (hello_per_object_motion_blur.cpp, draw_triangle_velocity_tile :391-455), 9 (hello_depth_of_field.cpp :524-574) or 10
// (hello_ping_pong.cpp :352-400), tile jobs of 80.  Their depth plane is then in screen rows.  The whole frame is
//   raster.process(dt);
//   chain.object_blur(blur_desc, frame_dev);  // hello_per_object_motion_blur.cpp; the frame is frame_dev
//   chain.dof(dof_desc);                      // hello_depth_of_field.cpp; the frame is the colour plane
//   chain.ping_pong(W, H);                    // hello_ping_pong.cpp; the frame is the colour plane
// Uncompiled, like the other seams.
// -----------------------------------------------------------------------------------------------------
template <class SceneT>
class MotionRasterGPU : public shs::AbstractSystem {
public:
    MotionRasterGPU(SceneT *scene, Device *dev, bool star, float max_velocity_px, int tile = 80)
        : scene_(scene), dev_(dev), star_(star), max_px_(max_velocity_px), tile_(tile) {}

    std::vector<typename RenderTargetSystemGPU<SceneT>::Object> objects;     // model / prev_model per frame

    void process(float) override {
        shs::Canvas &canvas = *scene_->canvas;
        const int W = canvas.get_width(), H = canvas.get_height();
        const shs::Camera3D &cam = *scene_->viewer->camera;
        const glm::mat4 view = cam.view_matrix, proj = cam.projection_matrix;
        std::vector<shs_rt_draw> draws(objects.size());
        for (size_t i = 0; i < objects.size(); ++i) {
            const auto &o = objects[i];
            shs_rt_draw &d = draws[i];
            d.mesh_id = o.mesh_id;
            d.albedo_tex = 0;
            const glm::mat4 mvp = proj * view * o.model, prev_mvp = prev_proj_ * prev_view_ * o.prev_model;
            std::memcpy(d.model, glm::value_ptr(o.model), 64);
            std::memcpy(d.mvp, glm::value_ptr(mvp), 64);
            std::memcpy(d.prev_mvp, glm::value_ptr(prev_mvp), 64);
            d.base_color[0] = o.base_color.r; d.base_color[1] = o.base_color.g; d.base_color[2] = o.base_color.b; d.base_color[3] = 255;
        }
        shs_rt_frame f{};
        f.width = W; f.height = H;
        f.ref_tile_w = star_ ? W : tile_;
        f.ref_tile_h = star_ ? H : tile_;
        std::memcpy(f.clear_color, clear_color, 4);
        std::memcpy(f.view, glm::value_ptr(view), 64);
        std::memcpy(f.light_dir_world, glm::value_ptr(light_dir_world), 12);
        std::memcpy(f.camera_pos, glm::value_ptr(scene_->viewer->position), 12);
        f.max_velocity_px = max_px_;
        f.shading = plain_shading ? plain_shading : star_ ? 7 : 6;
        if (plain_shading) ok(shs_rt_render_plain(dev_->ctx, &f, draws.data(), (int32_t)draws.size()));
        else ok(shs_rt_render_motion(dev_->ctx, &f, draws.data(), (int32_t)draws.size()));
        prev_view_ = view;
        prev_proj_ = proj;
    }

    void ok(int rc) const {
        if (rc != SHS_OK) throw std::runtime_error(shs_last_error(dev_->ctx));
    }

    glm::vec3 light_dir_world{-1.0f, -0.4f, 1.0f};   // (the shaders normalise it)
    uint8_t clear_color[4] = {20, 20, 25, 255};
    int plain_shading = 0;                           // 8, 9 or 10: one of the three plain demos (shs_rt_render_plain)

private:
    SceneT *scene_;
    Device *dev_;
    bool star_;
    float max_px_;
    int tile_;
    glm::mat4 prev_view_{1.0f}, prev_proj_{1.0f};
};

// =====================================================================================================
// Seam 3 -- the library's plugin pipeline (shs-renderer-lib/include/shs/pipeline/).
// =====================================================================================================
}  // namespace shs_gpu_seams

#if __has_include("shs/pipeline/pass_adapters.hpp")
#include "shs/pipeline/pass_adapters.hpp"
#include "shs/sky/cubemap_sky.hpp"

namespace shs_gpu_seams {

// Device-resident MeshData (resources/mesh.hpp:23-43), uploaded on first use.
class GpuMeshes {
public:
    explicit GpuMeshes(shs_ctx *ctx) : ctx_(ctx) {}
    int32_t id(const shs::MeshData &m) {
        auto it = ids_.find(&m);
        if (it != ids_.end()) return it->second;
        int32_t id = -1;
        check(ctx_, shs_mesh_upload(ctx_, glm::value_ptr(m.positions[0]), static_cast<int32_t>(m.positions.size()),
                                    m.normals.empty() ? nullptr : glm::value_ptr(m.normals[0]),
                                    static_cast<int32_t>(m.normals.size()),
                                    m.uvs.empty() ? nullptr : glm::value_ptr(m.uvs[0]), static_cast<int32_t>(m.uvs.size()),
                                    m.indices.empty() ? nullptr : m.indices.data(), static_cast<int64_t>(m.indices.size()),
                                    &id));
        ids_.emplace(&m, id);
        return id;
    }

private:
    shs_ctx *ctx_;
    std::unordered_map<const shs::MeshData *, int32_t> ids_;
};

// Device-resident Texture2DData (resources/texture.hpp:23-49), uploaded on first use; an invalid one
// (Texture2DData::valid() false) maps to 0 -- the sampler's vec3(1) (builtin_shaders.hpp:35).
class GpuTextures {
public:
    explicit GpuTextures(shs_ctx *ctx) : ctx_(ctx) {}
    int32_t id(const shs::Texture2DData *t) {
        if (!t || !t->valid()) return 0;
        auto it = ids_.find(t);
        if (it != ids_.end()) return it->second;
        int32_t id = 0;
        check(ctx_, shs_texture_upload(ctx_, &t->texels[0].r, t->w, t->h, &id));
        ids_.emplace(t, id);
        return id;
    }

private:
    shs_ctx *ctx_;
    std::unordered_map<const shs::Texture2DData *, int32_t> ids_;
};

// The scene's sky models (sky/sky_model.hpp).  ISkyModel exposes only sample(), and ProceduralSky and
// CubemapSky keep their parameters private, so the host binds each model to the parameters it was built
// with, where it creates it; PassPBRForwardGPU looks scene.sky up here and adds the frame's camera.
class GpuSkies {
public:
    explicit GpuSkies(GpuTextures &textures) : textures_(textures) {}
    // ProceduralSky(sun_dir_ws) (sky/procedural_sky.hpp:22-24); call again after set_sun_direction
    void bind_procedural(const shs::ISkyModel *sky, const glm::vec3 &sun_dir_ws) {
        shs_sky_desc d{};
        d.model = SHS_SKY_PROCEDURAL;
        std::memcpy(d.sun_dir_ws, glm::value_ptr(sun_dir_ws), 12);
        skies_[sky] = d;
    }
    // CubemapSky(cubemap, intensity) (sky/cubemap_sky.hpp:76-78).  A cubemap that fails CubemapData::valid()
    // samples black everywhere: the model is bound as SHS_SKY_NONE with a black clear.
    void bind_cubemap(const shs::ISkyModel *sky, const shs::CubemapData &cubemap, float intensity) {
        shs_sky_desc d{};
        d.model = cubemap.valid() ? SHS_SKY_CUBEMAP : SHS_SKY_NONE;
        for (int k = 0; k < 6 && cubemap.valid(); ++k) d.face_tex[k] = textures_.id(&cubemap.face[(size_t)k]);
        d.intensity = intensity;
        skies_[sky] = d;
    }
    void unbind(const shs::ISkyModel *sky) { skies_.erase(sky); }
    const shs_sky_desc *find(const shs::ISkyModel *sky) const {
        const auto it = skies_.find(sky);
        return it == skies_.end() ? nullptr : &it->second;
    }

private:
    GpuTextures &textures_;
    std::unordered_map<const shs::ISkyModel *, shs_sky_desc> skies_;
};

// Shared by the passes of one pipeline: the device context, its meshes, textures and sky models, and
// whether the device shadow map belongs to the current frame.
struct GpuPassRuntime {
    Device device;
    GpuMeshes meshes;
    GpuTextures textures;
    GpuSkies skies;
    bool resolve_shadow_to_host = false;   // also fill RT_ShadowDepth (for CPU consumers: shadow debug)
    explicit GpuPassRuntime(int device_index = 0)
        : device(device_index), meshes(device.ctx), textures(device.ctx), skies(textures) {}
};

// RenderItem transform, as both passes build it (pass_shadow_map.hpp:56-64, pass_pbr_forward.hpp:136-141).
inline glm::mat4 item_model(const shs::RenderItem &item) {
    glm::mat4 model(1.0f);
    model = glm::translate(model, item.tr.pos);
    model = glm::rotate(model, item.tr.rot_euler.x, glm::vec3(1.0f, 0.0f, 0.0f));
    model = glm::rotate(model, item.tr.rot_euler.y, glm::vec3(0.0f, 1.0f, 0.0f));
    model = glm::rotate(model, item.tr.rot_euler.z, glm::vec3(0.0f, 0.0f, 1.0f));
    model = glm::scale(model, item.tr.scl);
    return model;
}

// PassShadowMap::execute (passes/pass_shadow_map.hpp:44-206) on the GPU: scene AABB of the casters'
// mesh bounds, build_dir_light_camera_aabb (camera/light_camera.hpp:33-98), the depth pass.  Sets
// ctx.shadow exactly as the CPU pass does; the depth map stays on the device for PassPBRForwardGPU.
class PassShadowMapGPU final : public shs::IRenderPass {
public:
    PassShadowMapGPU(std::shared_ptr<GpuPassRuntime> rt, shs::RT_Shadow rt_shadow) : rt_(std::move(rt)), rt_shadow_(rt_shadow) {}

    const char *id() const override { return "shadow_map"; }
    shs::RenderBackendType preferred_backend() const override { return shs::RenderBackendType::Software; }
    bool supports_backend(shs::RenderBackendType b) const override { return b == shs::RenderBackendType::Software; }
    shs::TechniquePassContract describe_contract() const override { return shs::PassShadowMapAdapter(rt_shadow_).describe_contract(); }
    shs::PassIODesc describe_io() const override { return shs::PassShadowMapAdapter(rt_shadow_).describe_io(); }

    shs::PassExecutionResult execute_resolved(shs::Context &ctx, const shs::PassExecutionRequest &request) override {
        if (!request.valid || !request.inputs.scene || !request.inputs.frame || !request.inputs.registry)
            return shs::PassExecutionResult::not_executed();
        const shs::Scene &scene = *request.inputs.scene;
        const shs::FrameParams &fp = *request.inputs.frame;
        ctx.shadow.reset();
        if (!rt_shadow_.valid() || !fp.pass.shadow.enable) return shs::PassExecutionResult::executed_no_outputs();
        auto *shadow = static_cast<shs::RT_ShadowDepth *>(request.inputs.registry->get(rt_shadow_));
        if (!shadow || shadow->w <= 0 || shadow->h <= 0) return shs::PassExecutionResult::executed_no_outputs();

        casters_.clear();
        for (const auto &item : scene.items) {
            if (!item.visible || !item.casts_shadow || !scene.resources) continue;
            const shs::MeshData *mesh = scene.resources->get_mesh((shs::MeshAssetHandle)item.mesh);
            if (!mesh || mesh->positions.empty()) continue;
            shs_shadow_caster c{};
            c.mesh_id = rt_->meshes.id(*mesh);
            const glm::mat4 model = item_model(item);
            std::memcpy(c.model, glm::value_ptr(model), sizeof c.model);
            casters_.push_back(c);
        }
        shs_ctx *dctx = rt_->device.ctx;
        float light_vp[16];
        check(dctx, shs_render_shadow_map(dctx, shadow->w, shadow->h, glm::value_ptr(scene.sun.dir_ws), casters_.data(),
                                          static_cast<int32_t>(casters_.size()), light_vp));
        ctx.shadow.map = shadow;
        ctx.shadow.light_viewproj = glm::make_mat4(light_vp);
        ctx.shadow.valid = true;
        if (rt_->resolve_shadow_to_host) check(dctx, shs_resolve_shadow_map(dctx, shadow->depth.data()));
        return shs::PassExecutionResult::executed_no_outputs();
    }

private:
    std::shared_ptr<GpuPassRuntime> rt_;
    shs::RT_Shadow rt_shadow_{};
    std::vector<shs_shadow_caster> casters_;
};

// PassPBRForward::execute (passes/pass_pbr_forward.hpp:49-214) on the GPU: one shs_lib_draw per visible
// item with the ShaderUniforms the pass builds, the program it binds (:100-108), the motion history
// (:123-155), then one resolve into RT_ColorHDR / RT_ColorDepthMotion (PixelBuffer2D rows, y up).
class PassPBRForwardGPU final : public shs::IRenderPass {
public:
    PassPBRForwardGPU(std::shared_ptr<GpuPassRuntime> rt, shs::RTHandle rt_hdr, shs::RT_Motion rt_motion, shs::RTHandle rt_shadow)
        : rt_(std::move(rt)), rt_hdr_(rt_hdr), rt_motion_(rt_motion), rt_shadow_(rt_shadow) {}

    const char *id() const override { return "pbr_forward"; }
    shs::RenderBackendType preferred_backend() const override { return shs::RenderBackendType::Software; }
    bool supports_backend(shs::RenderBackendType b) const override { return b == shs::RenderBackendType::Software; }
    shs::TechniquePassContract describe_contract() const override {
        return shs::PassPBRForwardAdapter(rt_hdr_, rt_motion_, rt_shadow_).describe_contract();
    }
    shs::PassIODesc describe_io() const override { return shs::PassPBRForwardAdapter(rt_hdr_, rt_motion_, rt_shadow_).describe_io(); }

    shs::PassExecutionResult execute_resolved(shs::Context &ctx, const shs::PassExecutionRequest &request) override {
        if (!request.valid || !request.inputs.scene || !request.inputs.frame || !request.inputs.registry)
            return shs::PassExecutionResult::not_executed();
        const shs::Scene &scene = *request.inputs.scene;
        const shs::FrameParams &fp = *request.inputs.frame;
        shs::RTRegistry &rtr = *request.inputs.registry;
        if (!rt_hdr_.valid()) return shs::PassExecutionResult::not_executed();
        auto *hdr = static_cast<shs::RT_ColorHDR *>(rtr.get(rt_hdr_));
        if (!hdr || hdr->w <= 0 || hdr->h <= 0) return shs::PassExecutionResult::not_executed();
        auto *motion = rt_motion_.valid() ? static_cast<shs::RT_ColorDepthMotion *>(rtr.get(rt_motion_)) : nullptr;
        auto *shadow = rt_shadow_.valid() ? static_cast<shs::RT_ShadowDepth *>(rtr.get(rt_shadow_)) : nullptr;
        const bool depth_motion = motion && motion->w == hdr->w && motion->h == hdr->h;
        // The background (:64-85): render_skybox_to_hdr of the scene's sky model, bound in rt_->skies with
        // the parameters it was created with, else the gradient.  A model nobody bound fails loudly.
        shs_sky_desc sky{};
        bool black_sky = false;   // an invalid cubemap: CubemapSky::sample returns vec3(0)
        if (scene.sky) {
            const shs_sky_desc *bound = rt_->skies.find(scene.sky);
            if (!bound) unsupported("sky models not bound with GpuPassRuntime::skies");
            sky = *bound;
            black_sky = sky.model == SHS_SKY_NONE;
            std::memcpy(sky.cam_viewproj, glm::value_ptr(scene.cam.viewproj), 64);
            std::memcpy(sky.cam_pos, glm::value_ptr(scene.cam.pos), 12);
        }

        int32_t program = SHS_PROGRAM_PBR_MR;
        if (fp.shading_model == shs::ShadingModel::BlinnPhong) program = SHS_PROGRAM_BLINN_PHONG;
        if (fp.debug_view == shs::DebugViewMode::Albedo) program = SHS_PROGRAM_DEBUG_ALBEDO;
        if (fp.debug_view == shs::DebugViewMode::Normal) program = SHS_PROGRAM_DEBUG_NORMAL;
        if (fp.debug_view == shs::DebugViewMode::Depth) program = SHS_PROGRAM_DEBUG_DEPTH;
        const int32_t cull = fp.cull_mode == shs::CullMode::None    ? SHS_CULL_NONE
                             : fp.cull_mode == shs::CullMode::Front ? SHS_CULL_FRONT
                                                                    : SHS_CULL_BACK;

        std::unordered_map<uint64_t, glm::mat4> next_prev{};
        draws_.clear();
        for (size_t item_index = 0; item_index < scene.items.size(); ++item_index) {
            const auto &item = scene.items[item_index];
            if (!item.visible || !scene.resources) continue;
            const shs::MeshData *mesh = scene.resources->get_mesh((shs::MeshAssetHandle)item.mesh);
            if (!mesh || mesh->empty()) continue;
            const shs::MaterialData *mat = scene.resources->get_material((shs::MaterialAssetHandle)item.mat);
            // u.base_color_tex (:173-176): the registry's Texture2DData, sampled on the device
            const int32_t tex_id = (mat && mat->base_color_tex != 0)
                                       ? rt_->textures.id(scene.resources->get_texture(mat->base_color_tex))
                                       : 0;
            const glm::mat4 model = item_model(item);
            uint64_t key = item.object_id;                                         // :143-148
            if (key == 0) {
                key = ((uint64_t)item.mesh << 32) ^ (uint64_t)item.mat ^ ((uint64_t)item_index + 1u);
                if (key == 0) key = 1;
            }
            glm::mat4 prev_model = model;
            const auto it = ctx.history.prev_model_by_object.find(key);
            if (ctx.history.has_prev_frame && it != ctx.history.prev_model_by_object.end()) prev_model = it->second;
            next_prev[key] = model;

            shs_lib_draw d{};
            d.mesh_id = rt_->meshes.id(*mesh);
            d.program = program;
            d.cull_mode = cull;
            d.front_face_ccw = fp.front_face_ccw ? 1 : 0;
            const glm::mat4 prev_vp = ctx.history.has_prev_frame ? scene.cam.prev_viewproj : scene.cam.viewproj;
            std::memcpy(d.model, glm::value_ptr(model), 64);
            std::memcpy(d.viewproj, glm::value_ptr(scene.cam.viewproj), 64);
            std::memcpy(d.prev_model, glm::value_ptr(prev_model), 64);
            std::memcpy(d.prev_viewproj, glm::value_ptr(prev_vp), 64);
            std::memcpy(d.light_dir_ws, glm::value_ptr(scene.sun.dir_ws), 12);
            std::memcpy(d.light_color, glm::value_ptr(scene.sun.color), 12);
            d.light_intensity = scene.sun.intensity;
            std::memcpy(d.camera_pos, glm::value_ptr(scene.cam.pos), 12);
            const glm::vec3 base = mat ? mat->base_color : glm::vec3(0.8f, 0.5f, 0.2f);   // :175-181
            std::memcpy(d.base_color, glm::value_ptr(base), 12);
            d.metallic = mat ? mat->metallic : 0.1f;
            d.roughness = mat ? mat->roughness : 0.5f;
            d.ao = mat ? mat->ao : 1.0f;
            if (fp.pass.shadow.enable && shadow && ctx.shadow.valid) {                    // :184-193
                d.shadow = 1;
                std::memcpy(d.light_viewproj, glm::value_ptr(ctx.shadow.light_viewproj), 64);
                d.shadow_bias_const = fp.pass.shadow.bias_const;
                d.shadow_bias_slope = fp.pass.shadow.bias_slope;
                d.shadow_pcf_radius = fp.pass.shadow.pcf_radius;
                d.shadow_pcf_step = fp.pass.shadow.pcf_step;
                d.shadow_strength = fp.pass.shadow.strength;
            }
            d.enable_motion_vectors = fp.pass.motion_vectors.enable ? 1 : 0;
            d.base_color_tex = tex_id;
            draws_.push_back(d);
        }

        shs_lib_frame f{};
        f.width = hdr->w;
        f.height = hdr->h;
        f.shard_rank = 0;
        f.shard_count = 1;
        f.flags = (black_sky ? 0u : SHS_LIB_BG_GRADIENT) | (depth_motion ? SHS_LIB_DEPTH_MOTION : 0u);
        f.clear_hdr[3] = 1.0f;   // black_sky: (0, 0, 0, 1)
        f.zn = depth_motion ? motion->zn : 0.1f;
        f.zf = depth_motion ? motion->zf : 1000.0f;
        shs_ctx *dctx = rt_->device.ctx;
        check(dctx, shs_lib_set_sky(dctx, scene.sky ? &sky : nullptr));
        check(dctx, shs_render_pbr_forward(dctx, &f, draws_.data(), static_cast<int32_t>(draws_.size())));
        check(dctx, shs_resolve_lib(dctx, &hdr->color.data[0].r, depth_motion ? motion->depth.data.data() : nullptr,
                                    depth_motion ? &motion->motion.data[0].x : nullptr));
        shs_lib_stats st{};
        check(dctx, shs_get_lib_stats(dctx, &st));
        ctx.debug.tri_input = st.tri_input;
        ctx.debug.tri_after_clip = st.tri_after_clip;
        ctx.debug.tri_raster = st.tri_raster;
        ctx.history.prev_model_by_object.swap(next_prev);
        ctx.history.has_prev_frame = true;
        return shs::PassExecutionResult::executed_no_outputs();
    }

private:
    // Inputs outside the GPU pass's scope (DESIGN.md "Out of scope") fail loudly: no silent CPU path.
    [[noreturn]] static void unsupported(const char *what) {
        throw std::runtime_error(std::string("PassPBRForwardGPU: ") + what + " are not supported on the GPU path");
    }

    std::shared_ptr<GpuPassRuntime> rt_;
    shs::RTHandle rt_hdr_{};
    shs::RT_Motion rt_motion_{};
    shs::RTHandle rt_shadow_{};
    std::vector<shs_lib_draw> draws_;
};

// Replace the standard registry's "shadow_map" and "pbr_forward" factories with the GPU passes
// (PassFactoryRegistry::register_factory overwrites by id, pass_registry.hpp:52-63); every other pass
// keeps the reference's implementation.  Usage:
//   auto reg = shs::make_standard_pass_factory_registry(rt_shadow, rt_hdr, rt_motion, rt_ldr, t0, t1);
//   auto gpu = std::make_shared<shs_gpu_seams::GpuPassRuntime>(0);
//   shs_gpu_seams::register_gpu_passes(reg, gpu, rt_shadow, rt_hdr, rt_motion);
inline void register_gpu_passes(shs::PassFactoryRegistry &reg, std::shared_ptr<GpuPassRuntime> rt, shs::RT_Shadow rt_shadow,
                                shs::RTHandle rt_hdr, shs::RT_Motion rt_motion) {
    reg.register_factory(shs::PassId::ShadowMap, [=]() { return std::make_unique<PassShadowMapGPU>(rt, rt_shadow); });
    reg.register_factory(shs::PassId::PBRForward, [=]() {
        return std::make_unique<PassPBRForwardGPU>(rt, rt_hdr, rt_motion, shs::RTHandle{rt_shadow.id});
    });
}

}  // namespace shs_gpu_seams

// ---- typed local lights (SHS_PROGRAM_FORWARD_PLUS_TYPED) ------------------------------------------
#include "shs/lighting/light_runtime.hpp"

namespace shs_gpu_seams {

// LightProperties (lighting/light_runtime.hpp:53-72) of a light of `type` as the record
// shs_light_pack_culling / shs_lights_upload_typed take (exp-plumbing/hello_light_types_culling_sw.cpp:
// one per LightInstance, type = light.model->type()).
inline shs_light_props to_shs_light_props(const shs::LightProperties &p, shs::LightType type) {
    shs_light_props o{};
    o.type = static_cast<uint32_t>(type);
    o.attenuation_model = static_cast<uint32_t>(p.attenuation_model);
    o.flags = p.flags;
    o.range = p.range;
    std::memcpy(o.position_ws, glm::value_ptr(p.position_ws), 12);
    o.intensity = p.intensity;
    std::memcpy(o.color, glm::value_ptr(p.color), 12);
    o.inner_angle_rad = p.inner_angle_rad;
    std::memcpy(o.direction_ws, glm::value_ptr(p.direction_ws), 12);
    o.outer_angle_rad = p.outer_angle_rad;
    std::memcpy(o.right_ws, glm::value_ptr(p.right_ws), 12);
    o.tube_half_length = p.tube_half_length;
    std::memcpy(o.up_ws, glm::value_ptr(p.up_ws), 12);
    o.tube_radius = p.tube_radius;
    o.rect_half_extents[0] = p.rect_half_extents.x;
    o.rect_half_extents[1] = p.rect_half_extents.y;
    o.attenuation_power = p.attenuation_power;
    o.attenuation_bias = p.attenuation_bias;
    o.attenuation_cutoff = p.attenuation_cutoff;
    return o;
}

}  // namespace shs_gpu_seams
#endif
