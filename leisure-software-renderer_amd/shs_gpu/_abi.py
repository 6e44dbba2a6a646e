"""ctypes declarations of include/shs_gpu.h (libshs_gpu.so, built in-tree for gfx950).

The product path: every call goes through the C ABI into the HIP kernels.  There is no CPU
fallback -- if the shared library is missing or fails to load, importing this module raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SHS_GPU_LIB: another in-tree build of the library (timing experiments with compile-time variants)
LIB_PATH = os.environ.get("SHS_GPU_LIB") or os.path.join(HERE, "libshs_gpu.so")

SHS_OK = 0
SHS_ERR_INVALID = -1
SHS_ERR_HIP = -2
SHS_ERR_NO_DEVICE = -3
SHS_ERR_OVERFLOW = -4

SHADING_FLAT = 0
SHADING_GOURAUD = 1
SHADING_PHONG = 2
SHADING_BLINN_PHONG = 3
SHADING_TOON = 4
SHADING_GOOCH = 5
SHADING_OREN_NAYAR = 6
SHADING_NORMAL_VIS = 7
SHADING_DEPTH_VIS = 8
SHADING_TEXTURED = 9
# (the models a scene of meshes and Uniforms alone can draw; SHADING_TEXTURED also needs UVs and a texture)
SHADING_NAMES = {"flat": 0, "gouraud": 1, "phong": 2, "blinn_phong": 3, "toon": 4, "gooch": 5, "oren_nayar": 6,
                 "normal_vis": 7, "depth_vis": 8}

FRAME_PREQUANT = 1
FRAME_PRESENT = 2
OPT_BIN_CAPACITY = 1
OPT_RASTER_MODE = 2
OPT_TIMELINE = 3
OPT_RASTER_LOOP = 4
OPT_SPILL_CAPACITY = 5
OPT_FRAG_CAPACITY = 6
OPT_LIB_PART = 7
OPT_SHARD_CULL = 8
OPT_SHARD_LAYOUT = 9
SHARD_INTERLEAVED = 0
SHARD_REGIONS = 1
OPT_SHARD_ROOT_SHARE = 10
OPT_SHADOW_FOOTPRINT = 11
OPT_LEGACY_PIPELINE = 12
OPT_LEGACY_STALE_CLEAR = 13
OPT_LEGACY_TILE_GROUPS = 14
OPT_LEGACY_GROUP_SPANS = 15


class LegacyDraw(ctypes.Structure):
    _fields_ = [
        ("mesh_id", ctypes.c_int32),
        ("shading", ctypes.c_int32),
        ("mvp", ctypes.c_float * 16),
        ("model", ctypes.c_float * 16),
        ("light_dir", ctypes.c_float * 3),
        ("camera_pos", ctypes.c_float * 3),
        ("color", ctypes.c_uint8 * 4),
    ]


class FrameDesc(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("ref_tile_w", ctypes.c_int32),
        ("ref_tile_h", ctypes.c_int32),
        ("shard_rank", ctypes.c_int32),
        ("shard_count", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("clear_color", ctypes.c_uint8 * 4),
    ]


class RasterStats(ctypes.Structure):
    _fields_ = [
        ("tri_input", ctypes.c_uint64),
        ("tri_setup", ctypes.c_uint64),
        ("tri_ghost", ctypes.c_uint64),
        ("bin_entries", ctypes.c_uint64),
        ("covered_pixels", ctypes.c_uint64),
        ("tri_ghost_unbounded", ctypes.c_uint64),
        ("spilled", ctypes.c_uint64),
        ("max_tile_bin", ctypes.c_uint64),
        ("ghost_fragments", ctypes.c_uint64),
    ]


# ---- library path (rasterize_mesh / PassShadowMap / PassPBRForward) ----
PROGRAM_PBR_MR = 0
PROGRAM_BLINN_PHONG = 1
PROGRAM_DEBUG_ALBEDO = 2
PROGRAM_DEBUG_NORMAL = 3
PROGRAM_DEBUG_DEPTH = 4
CULL_NONE, CULL_BACK, CULL_FRONT = 0, 1, 2
LIB_DEPTH_MOTION = 1
LIB_BG_GRADIENT = 2

_F16 = ctypes.c_float * 16
_F3 = ctypes.c_float * 3


class LibDrawC(ctypes.Structure):
    _fields_ = [
        ("mesh_id", ctypes.c_int32),
        ("program", ctypes.c_int32),
        ("cull_mode", ctypes.c_int32),
        ("front_face_ccw", ctypes.c_int32),
        ("model", _F16), ("viewproj", _F16), ("prev_model", _F16), ("prev_viewproj", _F16),
        ("light_dir_ws", _F3), ("light_color", _F3), ("light_intensity", ctypes.c_float), ("camera_pos", _F3),
        ("base_color", _F3), ("metallic", ctypes.c_float), ("roughness", ctypes.c_float), ("ao", ctypes.c_float),
        ("shadow", ctypes.c_int32),
        ("light_viewproj", _F16),
        ("shadow_bias_const", ctypes.c_float), ("shadow_bias_slope", ctypes.c_float),
        ("shadow_pcf_radius", ctypes.c_int32),
        ("shadow_pcf_step", ctypes.c_float), ("shadow_strength", ctypes.c_float),
        ("enable_motion_vectors", ctypes.c_int32),
        ("base_color_tex", ctypes.c_int32),
    ]


class LibFrameC(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("shard_rank", ctypes.c_int32), ("shard_count", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("zn", ctypes.c_float), ("zf", ctypes.c_float),
        ("clear_hdr", ctypes.c_float * 4),
    ]


class LibStats(ctypes.Structure):
    _fields_ = [
        ("tri_input", ctypes.c_uint64), ("tri_after_clip", ctypes.c_uint64), ("tri_raster", ctypes.c_uint64),
        ("covered_pixels", ctypes.c_uint64), ("max_tile_bin", ctypes.c_uint64), ("spilled", ctypes.c_uint64),
        ("clipped_extra", ctypes.c_uint64),
    ]


class ShadowCasterC(ctypes.Structure):
    _fields_ = [("mesh_id", ctypes.c_int32), ("model", _F16)]


PROGRAM_FORWARD_PLUS = 5
TONEMAP_LDR, TONEMAP_PRESENT = 1, 2


MOTION_BLUR_PRESENT = 1


class MotionBlurDescC(ctypes.Structure):
    _fields_ = [("enable", ctypes.c_int32), ("samples", ctypes.c_int32), ("strength", ctypes.c_float),
                ("max_velocity_px", ctypes.c_float), ("min_velocity_px", ctypes.c_float),
                ("depth_reject", ctypes.c_float), ("dt", ctypes.c_float), ("flags", ctypes.c_uint32)]


LIGHT_SHAFTS_NO_DEPTH = 1


class LightShaftsDescC(ctypes.Structure):
    _fields_ = [("enable", ctypes.c_int32), ("steps", ctypes.c_int32), ("density", ctypes.c_float),
                ("weight", ctypes.c_float), ("decay", ctypes.c_float), ("cam_pos", _F3), ("sun_dir_ws", _F3),
                ("viewproj", _F16), ("flags", ctypes.c_uint32)]


SKY_NONE, SKY_PROCEDURAL, SKY_CUBEMAP = 0, 1, 2


class SkyDescC(ctypes.Structure):
    _fields_ = [("model", ctypes.c_int32), ("cam_viewproj", _F16), ("cam_pos", _F3), ("sun_dir_ws", _F3),
                ("face_tex", ctypes.c_int32 * 6), ("intensity", ctypes.c_float)]


class OccluderC(ctypes.Structure):
    _fields_ = [("mesh_id", ctypes.c_int32), ("model", _F16), ("aabb_min", _F3), ("aabb_max", _F3)]


class OcclusionDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("view", _F16), ("view_proj", _F16),
                ("depth_epsilon", ctypes.c_float), ("enable", ctypes.c_int32)]


class DebugDrawDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("view_proj", _F16), ("camera_pos", _F3),
                ("light_dir_ws", _F3)]


class DebugMeshC(ctypes.Structure):
    _fields_ = [("mesh_id", ctypes.c_int32), ("model", _F16), ("base_color", _F3)]


class DebugTriangleC(ctypes.Structure):
    _fields_ = [("p0", ctypes.c_float * 2), ("p1", ctypes.c_float * 2), ("p2", ctypes.c_float * 2), ("z", _F3),
                ("rgba", ctypes.c_uint8 * 4)]


class CanvasMotionBlurDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("curr_view", _F16), ("curr_proj", _F16),
                ("prev_view", _F16), ("prev_proj", _F16), ("samples", ctypes.c_int32), ("strength", ctypes.c_float),
                ("w_obj", ctypes.c_float), ("w_cam", ctypes.c_float), ("soft_knee", ctypes.c_int32),
                ("knee_px", ctypes.c_float), ("max_px", ctypes.c_float)]


class CanvasDofDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("blur_iterations", ctypes.c_int32),
                ("autofocus_radius", ctypes.c_int32), ("focus_x", ctypes.c_int32), ("focus_y", ctypes.c_int32),
                ("range", ctypes.c_float), ("max_blur", ctypes.c_float)]


class CanvasLightShaftsDescC(ctypes.Structure):
    """shs_canvas_light_shafts_desc: the pass's inputs, then LightShaftParams in its order (bools as int32)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("cam_pos", ctypes.c_float * 3),
                ("inv_view_proj", _F16), ("sun_dir_world", ctypes.c_float * 3), ("light_vp", _F16),
                ("shadow_w", ctypes.c_int32), ("shadow_h", ctypes.c_int32),
                ("enable", ctypes.c_int32), ("steps", ctypes.c_int32), ("max_dist", ctypes.c_float),
                ("min_dist", ctypes.c_float), ("base_density", ctypes.c_float), ("height_falloff", ctypes.c_float),
                ("noise_scale", ctypes.c_float), ("noise_strength", ctypes.c_float), ("jitter_amount", ctypes.c_float),
                ("ambient_strength", ctypes.c_float), ("sigma_s", ctypes.c_float), ("sigma_t", ctypes.c_float),
                ("g", ctypes.c_float), ("intensity", ctypes.c_float), ("use_shadow", ctypes.c_int32),
                ("shadow_bias", ctypes.c_float), ("shadow_pcf_2x2", ctypes.c_int32)]


CANVAS_LIGHT_SHAFTS_MAX_STEPS = 4096
CANVAS_MAX_OUTLINE_RADIUS = 4
CANVAS_MAX_FLARE_GHOSTS = 8
CANVAS_BLUR_VELOCITY_FIRST, CANVAS_BLUR_COMBINED_FIRST, CANVAS_BLUR_COMBINED_LATE = 0, 1, 2


class CanvasVelocityBlurDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("samples", ctypes.c_int32), ("strength", ctypes.c_float)]


class CanvasFogDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("fog_color", ctypes.c_uint8 * 4),
                ("fog_start", ctypes.c_float), ("fog_end", ctypes.c_float), ("fog_power", ctypes.c_float)]


class CanvasOutlineDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("radius", ctypes.c_int32),
                ("threshold", ctypes.c_float), ("strength", ctypes.c_float)]


class CanvasFxaaDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("reduce_min", ctypes.c_float),
                ("reduce_mul", ctypes.c_float), ("span_max", ctypes.c_float)]


class CanvasSpecBrightDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("threshold", ctypes.c_float),
                ("intensity", ctypes.c_float)]


class CanvasLensFlareDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("intensity", ctypes.c_float),
                ("halo_intensity", ctypes.c_float), ("chroma_shift_px", ctypes.c_float), ("n_ghosts", ctypes.c_int32),
                ("ghost_scales", ctypes.c_float * CANVAS_MAX_FLARE_GHOSTS)]


CANVAS_MAX_OBJECT_BLUR_SAMPLES = 64


class CanvasObjectBlurDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("multiplier", ctypes.c_float),
                ("velocity_scale", ctypes.c_float), ("min_vel2", ctypes.c_float), ("max_samples", ctypes.c_int32),
                ("depth_eps", ctypes.c_float), ("depth_rows", ctypes.c_int32)]


class CanvasMultiPassFrameDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("blur_mode", ctypes.c_int32),
                ("enable_dof", ctypes.c_int32), ("enable_fxaa", ctypes.c_int32),
                ("velocity_blur", CanvasVelocityBlurDescC), ("motion_blur", CanvasMotionBlurDescC), ("dof", CanvasDofDescC),
                ("fog", CanvasFogDescC), ("outline", CanvasOutlineDescC), ("fxaa", CanvasFxaaDescC)]


class CanvasGlowFrameDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("enable_dof", ctypes.c_int32),
                ("enable_bloom", ctypes.c_int32), ("enable_flare", ctypes.c_int32), ("bloom_iterations", ctypes.c_int32),
                ("velocity_blur", CanvasVelocityBlurDescC), ("dof", CanvasDofDescC), ("spec_bright", CanvasSpecBrightDescC),
                ("lens_flare", CanvasLensFlareDescC)]


RT_USE_SHADOW, RT_PCF, RT_PREQUANT = 1, 2, 4


class RtDrawC(ctypes.Structure):
    """shs_rt_draw: one object of the Canvas render-target passes."""
    _fields_ = [("mesh_id", ctypes.c_int32), ("albedo_tex", ctypes.c_int32), ("model", _F16), ("mvp", _F16),
                ("prev_mvp", _F16), ("base_color", ctypes.c_uint8 * 4)]


class RtFrameC(ctypes.Structure):
    """shs_rt_frame: the camera pass's frame-wide uniforms and constants."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ref_tile_w", ctypes.c_int32),
                ("ref_tile_h", ctypes.c_int32), ("clear_color", ctypes.c_uint8 * 4), ("view", _F16), ("light_vp", _F16),
                ("light_dir_world", _F3), ("camera_pos", _F3), ("bias_base", ctypes.c_float),
                ("bias_slope", ctypes.c_float), ("max_velocity_px", ctypes.c_float), ("flags", ctypes.c_uint32),
                ("shading", ctypes.c_int32)]


class RtPcssC(ctypes.Structure):
    """shs_rt_pcss: the PCSS constants of shs_rt_frame::shading 1."""
    _fields_ = [("light_uv_radius", ctypes.c_float), ("search_radius_texels", ctypes.c_float),
                ("min_filter_texels", ctypes.c_float), ("max_filter_texels", ctypes.c_float), ("epsilon", ctypes.c_float),
                ("blocker_samples", ctypes.c_int32), ("pcf_samples", ctypes.c_int32)]


class RtPbrDrawC(ctypes.Structure):
    """shs_rt_pbr_draw: hello_pbr.cpp's per-object uniforms beside shs_rt_draw."""
    _fields_ = [("normal_mat", ctypes.c_float * 9), ("metallic", ctypes.c_float), ("roughness", ctypes.c_float),
                ("ao", ctypes.c_float), ("ibl_diffuse_intensity", ctypes.c_float), ("ibl_specular_intensity", ctypes.c_float),
                ("ibl_reflection_strength", ctypes.c_float)]


class RtPbrC(ctypes.Structure):
    """shs_rt_pbr: the constants of fragment_shader_pbr."""
    _fields_ = [("exposure", ctypes.c_float), ("min_roughness", ctypes.c_float), ("direct_intensity", ctypes.c_float)]


RT_SKY_NONE, RT_SKY_ANALYTIC, RT_SKY_CUBEMAP = 0, 1, 2
RT_SKY_ENCODE_REINHARD, RT_SKY_ENCODE_CLAMP = 0, 1


class RtSkyC(ctypes.Structure):
    """shs_rt_sky: the legacy sky model and the camera of skybox_background_pass."""
    _fields_ = [("model", ctypes.c_int32), ("encode", ctypes.c_int32), ("sun_dir", _F3), ("intensity", ctypes.c_float),
                ("face_tex", ctypes.c_int32 * 6), ("cam_forward", _F3), ("cam_right", _F3), ("cam_up", _F3),
                ("fov_degrees", ctypes.c_float), ("exposure", ctypes.c_float)]


class RtSkyboxIblDrawC(ctypes.Structure):
    """shs_rt_skybox_ibl_draw: hello_ibl_skybox.cpp's per-object knobs beside shs_rt_draw (shading 4)."""
    _fields_ = [("ibl_ambient", ctypes.c_float), ("ibl_refl", ctypes.c_float), ("ibl_f0", ctypes.c_float),
                ("ibl_refl_mix", ctypes.c_float)]


class RtIblPhongDrawC(ctypes.Structure):
    """shs_rt_ibl_phong_draw: hello_ibl_skybox_optimized.cpp's / hello_ibl_skybox_xsimd.cpp's per-object knobs (shading 11)."""
    _fields_ = [("ibl_ambient", ctypes.c_float), ("ibl_refl", ctypes.c_float), ("ibl_f0", ctypes.c_float),
                ("ibl_refl_mix", ctypes.c_float), ("shininess", ctypes.c_float)]


RT_WATER_SURFACE = 1        # SHS_RT_WATER_SURFACE
RT_WATER_REFLECTION = 1     # SHS_RT_WATER_REFLECTION


class RtWaterDrawC(ctypes.Structure):
    """shs_rt_water_draw: which of hello_water.cpp's two fragment shaders a draw runs (shading 5)."""
    _fields_ = [("flags", ctypes.c_uint32)]


class RtWaterC(ctypes.Structure):
    """shs_rt_water: the frame's part of hello_water.cpp's Uniforms (:653-655)."""
    _fields_ = [("reflection_vp", _F16), ("time_sec", ctypes.c_float), ("flags", ctypes.c_uint32)]


class RtStatsC(ctypes.Structure):
    _fields_ = [("input_tris", ctypes.c_int64), ("polys3", ctypes.c_int64), ("polys4", ctypes.c_int64),
                ("sub_tris", ctypes.c_int64)]


class TonemapDescC(ctypes.Structure):
    _fields_ = [("exposure", ctypes.c_float), ("gamma", ctypes.c_float), ("flags", ctypes.c_uint32)]
LIGHT_CULL_NONE, LIGHT_CULL_TILED, LIGHT_CULL_TILED_DEPTH, LIGHT_CULL_CLUSTERED = 0, 1, 2, 3
_F4 = ctypes.c_float * 4


class CullingLightC(ctypes.Structure):
    """CullingLightGPU (lighting/light_types.hpp:141-166), 160 B."""
    _fields_ = [("position_range", _F4), ("color_intensity", _F4), ("direction_spot", _F4), ("axis_spot_outer", _F4),
                ("up_shape_x", _F4), ("shape_attenuation", _F4), ("type_shape_flags", ctypes.c_uint32 * 4),
                ("cull_sphere", _F4), ("cull_aabb_min", _F4), ("cull_aabb_max", _F4)]


PROGRAM_FORWARD_PLUS_TYPED = 6
LIGHT_POINT, LIGHT_SPOT, LIGHT_RECT_AREA, LIGHT_TUBE_AREA = 1, 2, 3, 4


class LightPropsC(ctypes.Structure):
    """shs_light_props: LightProperties (lighting/light_runtime.hpp:53-72) + its LightType, 128 B."""
    _fields_ = [("type", ctypes.c_uint32), ("attenuation_model", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("range", ctypes.c_float),
                ("position_ws", _F3), ("intensity", ctypes.c_float),
                ("color", _F3), ("inner_angle_rad", ctypes.c_float),
                ("direction_ws", _F3), ("outer_angle_rad", ctypes.c_float),
                ("right_ws", _F3), ("tube_half_length", ctypes.c_float),
                ("up_ws", _F3), ("tube_radius", ctypes.c_float),
                ("rect_half_extents", ctypes.c_float * 2), ("attenuation_power", ctypes.c_float),
                ("attenuation_bias", ctypes.c_float),
                ("attenuation_cutoff", ctypes.c_float), ("reserved", _F3)]


class LightCullDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("tile_size", ctypes.c_uint32),
                ("max_per_tile", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("z_slices", ctypes.c_uint32),
                ("view", _F16), ("proj", _F16), ("zn", ctypes.c_float), ("zf", ctypes.c_float),
                ("depth_linear", ctypes.c_int32), ("shard_rank", ctypes.c_int32), ("shard_count", ctypes.c_int32)]


class LightBinDescC(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("tile_size", ctypes.c_uint32),
                ("mode", ctypes.c_uint32), ("z_slices", ctypes.c_uint32), ("max_per_bin", ctypes.c_uint32),
                ("view_proj", _F16), ("z_near", ctypes.c_float), ("z_far", ctypes.c_float),
                ("tile_min_view_depth", ctypes.c_void_p), ("tile_max_view_depth", ctypes.c_void_p),
                ("n_depth_tiles", ctypes.c_int32)]


# (name, restype, argtypes) for every symbol include/shs_gpu.h declares.
_P = ctypes.c_void_p
_F = ctypes.POINTER(ctypes.c_float)
SIGNATURES = [
    ("shs_abi_version", ctypes.c_int, []),
    ("shs_gpu_tile_size", ctypes.c_int, []),
    ("shs_create", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_P)]),
    ("shs_destroy", ctypes.c_int, [_P]),
    ("shs_last_error", ctypes.c_char_p, [_P]),
    ("shs_set_stream", ctypes.c_int, [_P, _P]),
    ("shs_get_stream", _P, [_P]),
    ("shs_synchronize", ctypes.c_int, [_P]),
    ("shs_mesh_upload_soup", ctypes.c_int, [_P, _F, _F, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_mesh_upload_soup_uv", ctypes.c_int, [_P, _F, _F, _F, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_mesh_share", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_mesh_release", ctypes.c_int, [_P, ctypes.c_int32]),
    ("shs_render_legacy", ctypes.c_int, [_P, ctypes.POINTER(FrameDesc), ctypes.POINTER(LegacyDraw), ctypes.c_int32]),
    ("shs_render_legacy_batch", ctypes.c_int, [_P, ctypes.POINTER(FrameDesc), ctypes.POINTER(LegacyDraw), ctypes.c_int32,
                                               ctypes.c_int32]),
    ("shs_render_legacy_batch_tex", ctypes.c_int, [_P, ctypes.POINTER(FrameDesc), ctypes.POINTER(LegacyDraw),
                                                    ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32]),
    ("shs_legacy_sample_nearest", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, _F, _P]),
    ("shs_legacy_shade_samples", ctypes.c_int, [_P, ctypes.POINTER(LegacyDraw), ctypes.c_int32, _F, _F, _F, _P, _P]),
    ("shs_resolve", ctypes.c_int, [_P, _P, _P]),
    ("shs_resolve_frame", ctypes.c_int, [_P, ctypes.c_int32, _P, _P]),
    ("shs_resolve_present", ctypes.c_int, [_P, ctypes.c_int32, _P, ctypes.c_int32]),
    ("shs_present_device", ctypes.c_int, [_P, ctypes.c_int32, ctypes.POINTER(_P)]),
    ("shs_resolve_prequant", ctypes.c_int, [_P, _P]),
    ("shs_resolve_prequant_frame", ctypes.c_int, [_P, ctypes.c_int32, _P]),
    ("shs_texture_upload", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_texture_release", ctypes.c_int, [_P, ctypes.c_int32]),
    ("shs_device_framebuffers", ctypes.c_int, [_P, ctypes.POINTER(_P), ctypes.POINTER(_P)]),
    ("shs_get_stats", ctypes.c_int, [_P, ctypes.POINTER(RasterStats)]),
    ("shs_legacy_cleared_tiles", ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    ("shs_enable_timing", ctypes.c_int, [_P, ctypes.c_int]),
    ("shs_last_kernel_ms", ctypes.c_int, [_P, _F]),
    ("shs_timing_reset", ctypes.c_int, [_P]),
    ("shs_timing_read", ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    ("shs_debug_records", ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    ("shs_set_option", ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int64]),
    ("shs_debug_timeline", ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    ("shs_lib_debug_timeline", ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    ("shs_lib_debug_setup_timeline", ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    ("shs_tonemap", ctypes.c_int, [_P, ctypes.POINTER(TonemapDescC)]),
    ("shs_lib_fuse_tonemap", ctypes.c_int, [_P, ctypes.POINTER(TonemapDescC)]),
    ("shs_lib_set_sky", ctypes.c_int, [_P, ctypes.POINTER(SkyDescC)]),
    ("shs_sky_sample", ctypes.c_int, [_P, ctypes.POINTER(SkyDescC), _F, ctypes.c_int32, _F]),
    ("shs_resolve_ldr", ctypes.c_int, [_P, _P, _P]),
    ("shs_ldr_device_targets", ctypes.c_int, [_P, ctypes.POINTER(_P), ctypes.POINTER(_P)]),
    ("shs_tonemap_thresholds", ctypes.c_int, [ctypes.c_float, _F]),
    ("shs_occlusion_pass", ctypes.c_int, [_P, ctypes.POINTER(OcclusionDescC), ctypes.POINTER(OccluderC), ctypes.c_int32,
                                          _P, ctypes.c_int32, _P, _P, ctypes.POINTER(ctypes.c_int32), _P]),
    ("shs_debug_draw_meshes", ctypes.c_int, [_P, ctypes.POINTER(DebugDrawDescC), ctypes.POINTER(DebugMeshC), ctypes.c_int32,
                                             _P, _P, _P]),
    ("shs_debug_fill_triangles", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(DebugTriangleC),
                                                ctypes.c_int32, _P, _P]),
    ("shs_canvas_motion_blur", ctypes.c_int, [_P, ctypes.POINTER(CanvasMotionBlurDescC), _P, _P, _P, _P, ctypes.c_uint32]),
    ("shs_canvas_gaussian_blur", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.c_int32, ctypes.c_uint32]),
    ("shs_canvas_dof", ctypes.c_int, [_P, ctypes.POINTER(CanvasDofDescC), _P, _P, _P, _F, ctypes.c_uint32]),
    ("shs_canvas_light_shafts", ctypes.c_int, [_P, ctypes.POINTER(CanvasLightShaftsDescC), _P, _P, _P, _P, _P, ctypes.c_uint32]),
    ("shs_canvas_velocity_blur", ctypes.c_int, [_P, ctypes.POINTER(CanvasVelocityBlurDescC), _P, _P, _P, ctypes.c_uint32]),
    ("shs_canvas_fog", ctypes.c_int, [_P, ctypes.POINTER(CanvasFogDescC), _P, _P, _P, _P, ctypes.c_uint32]),
    ("shs_canvas_outline", ctypes.c_int, [_P, ctypes.POINTER(CanvasOutlineDescC), _P, _P, _P, ctypes.c_uint32]),
    ("shs_canvas_fxaa", ctypes.c_int, [_P, ctypes.POINTER(CanvasFxaaDescC), _P, _P, ctypes.c_uint32]),
    ("shs_canvas_spec_bright", ctypes.c_int, [_P, ctypes.POINTER(CanvasSpecBrightDescC), _P, _P, ctypes.c_uint32]),
    ("shs_canvas_additive", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.c_float, _P, ctypes.c_uint32]),
    ("shs_canvas_lens_flare", ctypes.c_int, [_P, ctypes.POINTER(CanvasLensFlareDescC), _P, _P, _P, ctypes.c_uint32]),
    ("shs_canvas_multi_pass_frame", ctypes.c_int, [_P, ctypes.POINTER(CanvasMultiPassFrameDescC), _P, _P, _P, _P,
                                                   ctypes.c_uint32]),
    ("shs_canvas_glow_frame", ctypes.c_int, [_P, ctypes.POINTER(CanvasGlowFrameDescC), _P, _P, _P, _P, _P, ctypes.c_uint32]),
    ("shs_rt_device_shadow_map", ctypes.c_int, [_P, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int32),
                                                ctypes.POINTER(ctypes.c_int32)]),
    ("shs_rt_render_shadow", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _F,
                                            ctypes.POINTER(RtDrawC), ctypes.c_int32]),
    ("shs_rt_render", ctypes.c_int, [_P, ctypes.POINTER(RtFrameC), ctypes.POINTER(RtDrawC), ctypes.c_int32]),
    ("shs_rt_set_pcss", ctypes.c_int, [_P, ctypes.POINTER(RtPcssC)]),
    ("shs_rt_pcss_samples", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P, _P]),
    ("shs_rt_set_pbr", ctypes.c_int, [_P, ctypes.POINTER(RtPbrC)]),
    ("shs_rt_set_ibl", ctypes.c_int, [_P, ctypes.c_int32, _P, ctypes.c_int32, ctypes.c_int32, _P]),
    ("shs_rt_render_pbr", ctypes.c_int, [_P, ctypes.POINTER(RtFrameC), ctypes.POINTER(RtDrawC), ctypes.POINTER(RtPbrDrawC),
                                         ctypes.c_int32]),
    ("shs_rt_render_pbr_soft", ctypes.c_int, [_P, ctypes.POINTER(RtFrameC), ctypes.POINTER(RtDrawC), ctypes.POINTER(RtPbrDrawC),
                                              ctypes.c_int32]),
    ("shs_rt_ibl_samples", ctypes.c_int, [_P, ctypes.c_int32, _P, _P, _P, _P]),
    ("shs_rt_render_skybox_ibl", ctypes.c_int, [_P, ctypes.POINTER(RtFrameC), ctypes.POINTER(RtDrawC),
                                                ctypes.POINTER(RtSkyboxIblDrawC), ctypes.c_int32]),
    ("shs_rt_render_ibl_phong", ctypes.c_int, [_P, ctypes.POINTER(RtFrameC), ctypes.POINTER(RtDrawC),
                                               ctypes.POINTER(RtIblPhongDrawC), ctypes.c_int32]),
    ("shs_rt_render_shadow_edge", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _F,
                                                 ctypes.POINTER(RtDrawC), ctypes.c_int32, ctypes.c_int32]),
    ("shs_rt_render_water", ctypes.c_int, [_P, ctypes.POINTER(RtFrameC), ctypes.POINTER(RtDrawC), ctypes.POINTER(RtWaterDrawC),
                                           ctypes.POINTER(RtWaterC), ctypes.c_int32]),
    ("shs_rt_render_motion", ctypes.c_int, [_P, ctypes.POINTER(RtFrameC), ctypes.POINTER(RtDrawC), ctypes.c_int32]),
    ("shs_rt_render_plain", ctypes.c_int, [_P, ctypes.POINTER(RtFrameC), ctypes.POINTER(RtDrawC), ctypes.c_int32]),
    ("shs_canvas_object_blur", ctypes.c_int, [_P, ctypes.POINTER(CanvasObjectBlurDescC), _P, _P, _P, _P, ctypes.c_uint32]),
    ("shs_canvas_ping_pong_blur", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_uint32]),
    ("shs_rt_resolve_spec", ctypes.c_int, [_P, _P]),
    ("shs_rt_device_spec", ctypes.c_int, [_P, ctypes.POINTER(_P)]),
    ("shs_rt_keep_reflection", ctypes.c_int, [_P]),
    ("shs_rt_set_reflection", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32]),
    ("shs_rt_water_samples", ctypes.c_int, [_P, ctypes.c_int32, _P, ctypes.c_float, _P, _P]),
    ("shs_rt_set_sky", ctypes.c_int, [_P, ctypes.POINTER(RtSkyC)]),
    ("shs_rt_sky_samples", ctypes.c_int, [_P, ctypes.c_int32, _P, _P]),
    ("shs_rt_resolve", ctypes.c_int, [_P, _P, _P, _P]),
    ("shs_rt_resolve_shadow", ctypes.c_int, [_P, _P]),
    ("shs_rt_resolve_prequant", ctypes.c_int, [_P, _P]),
    ("shs_rt_resolve_ids", ctypes.c_int, [_P, _P]),
    ("shs_rt_get_stats", ctypes.c_int, [_P, ctypes.POINTER(RtStatsC)]),
    ("shs_rt_device_targets", ctypes.c_int, [_P, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(_P)]),
    ("shs_ortho_lh_zo", ctypes.c_int, [ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_float, _F]),
    ("shs_motion_blur", ctypes.c_int, [_P, ctypes.POINTER(MotionBlurDescC)]),
    ("shs_resolve_motion_blur", ctypes.c_int, [_P, _P, _P]),
    ("shs_light_shafts", ctypes.c_int, [_P, ctypes.POINTER(LightShaftsDescC)]),
    ("shs_light_shafts_sun_uv", ctypes.c_int, [_F, _F, _F, _F, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_camera3d", ctypes.c_int, [_F, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _F, _F]),
    ("shs_model_trs", ctypes.c_int, [_F, ctypes.c_float, _F, _F]),
    ("shs_mat4_mul", ctypes.c_int, [_F, _F, _F]),
    ("shs_mat4_inverse", ctypes.c_int, [_F, _F]),
    ("shs_mesh_upload", ctypes.c_int, [_P, _F, ctypes.c_int32, _F, ctypes.c_int32, _F, ctypes.c_int32,
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_render_pbr_forward", ctypes.c_int, [_P, ctypes.POINTER(LibFrameC), ctypes.POINTER(LibDrawC), ctypes.c_int32]),
    ("shs_resolve_lib", ctypes.c_int, [_P, _P, _P, _P]),
    ("shs_get_lib_stats", ctypes.c_int, [_P, ctypes.POINTER(LibStats)]),
    ("shs_lib_device_targets", ctypes.c_int, [_P, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(_P)]),
    ("shs_lib_timing_reset", ctypes.c_int, [_P]),
    ("shs_lib_timing_read", ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    ("shs_render_shadow_map", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, _F, ctypes.POINTER(ShadowCasterC),
                                             ctypes.c_int32, _F]),
    ("shs_resolve_shadow_map", ctypes.c_int, [_P, _P]),
    ("shs_get_shadow_region", ctypes.c_int, [_P, _P]),
    ("shs_shadow_footprint", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int32, ctypes.c_int32, _P, _P, _P,
                                            ctypes.c_int32, _P]),
    ("shs_shadow_footprint_rows", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, _P, ctypes.c_int32, ctypes.c_int32, _P,
                                                 _P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P]),
    ("shs_tiles_packed_words", ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]),
    ("shs_tiles_rank_words", ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]),
    ("shs_get_shard_regions", ctypes.c_int, [_P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_shard_balance_rects", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_tiles_pack", ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, _P]),
    ("shs_tiles_unpack", ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, _P]),
    ("shs_tiles_unpack_ranks", ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    ("shs_lights_upload", ctypes.c_int, [_P, ctypes.POINTER(CullingLightC), ctypes.c_int32]),
    ("shs_light_pack_culling", ctypes.c_int, [ctypes.POINTER(LightPropsC), ctypes.c_int32, ctypes.POINTER(CullingLightC)]),
    ("shs_lights_upload_typed", ctypes.c_int, [_P, ctypes.POINTER(CullingLightC), ctypes.POINTER(LightPropsC), ctypes.c_int32]),
    ("shs_light_cull", ctypes.c_int, [_P, ctypes.POINTER(LightCullDescC)]),
    ("shs_light_bin_culling", ctypes.c_int, [_P, ctypes.POINTER(LightBinDescC), _P, ctypes.c_int32, _P, _P, _P]),
    ("shs_resolve_light_lists", ctypes.c_int, [_P, _P, _P, _P]),
    ("shs_look_at_lh", ctypes.c_int, [_F, _F, _F, _F]),
    ("shs_perspective_lh_no", ctypes.c_int, [ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _F]),
    ("shs_model_euler", ctypes.c_int, [_F, _F, _F, _F]),
    ("shs_dir_light_camera_aabb", ctypes.c_int, [_F, _F, _F, ctypes.c_float, ctypes.c_uint32, _F, _F, _F]),
    # multi-GPU from one host process
    ("shs_group_create", ctypes.c_int, [ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(_P)]),
    ("shs_group_destroy", ctypes.c_int, [_P]),
    ("shs_group_last_error", ctypes.c_char_p, [_P]),
    ("shs_group_size", ctypes.c_int, [_P]),
    ("shs_group_context", ctypes.c_int, [_P, ctypes.c_int32, ctypes.POINTER(_P)]),
    ("shs_group_mesh_upload", ctypes.c_int, [_P, _F, ctypes.c_int32, _F, ctypes.c_int32, _F, ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_uint32), ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_group_mesh_upload_soup", ctypes.c_int, [_P, _F, _F, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_group_mesh_upload_soup_uv", ctypes.c_int, [_P, _F, _F, _F, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_group_render_legacy_tex", ctypes.c_int, [_P, ctypes.POINTER(FrameDesc), ctypes.POINTER(LegacyDraw),
                                                    ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
    ("shs_group_texture_upload", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("shs_group_lights_upload", ctypes.c_int, [_P, ctypes.POINTER(CullingLightC), ctypes.c_int32]),
    ("shs_group_lights_upload_typed", ctypes.c_int, [_P, ctypes.POINTER(CullingLightC), ctypes.POINTER(LightPropsC),
                                                     ctypes.c_int32]),
    ("shs_group_set_option", ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int64]),
    ("shs_group_lib_fuse_tonemap", ctypes.c_int, [_P, ctypes.POINTER(TonemapDescC)]),
    ("shs_group_lib_set_sky", ctypes.c_int, [_P, ctypes.POINTER(SkyDescC)]),
    ("shs_group_light_cull", ctypes.c_int, [_P, ctypes.POINTER(LightCullDescC)]),
    ("shs_group_render_shadow_map", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, _F, ctypes.POINTER(ShadowCasterC),
                                                   ctypes.c_int32, _F]),
    ("shs_group_render_pbr_forward", ctypes.c_int, [_P, ctypes.POINTER(LibFrameC), ctypes.POINTER(LibDrawC), ctypes.c_int32]),
    ("shs_group_render_legacy", ctypes.c_int, [_P, ctypes.POINTER(FrameDesc), ctypes.POINTER(LegacyDraw), ctypes.c_int32]),
    ("shs_group_gather", ctypes.c_int, [_P, ctypes.c_int]),
    ("shs_group_synchronize", ctypes.c_int, [_P]),
]


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so /
    libhsa-runtime64.so and load them by file name from torch/lib; libshs_gpu.so asks the dynamic
    linker for the SONAMEs libamdhip64.so.7 / libhsa-runtime64.so.1.  If libshs_gpu.so is loaded first,
    the system ROCm runtime comes up, and a later `import torch` maps a second HIP + HSA runtime into
    the process whose device enumeration then fails ("No HIP GPUs are available" / hipErrorNoDevice:
    tools/diag_runtime.py).  Loading torch's runtime first (by path, RTLD_GLOBAL,
    without importing torch) makes libshs_gpu.so bind to it by SONAME, and torch later finds the same
    file already mapped.  Without torch the system runtime is used.  SHS_GPU_HIP_RUNTIME=system skips."""
    if os.environ.get("SHS_GPU_HIP_RUNTIME", "") == "system":
        return None
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.submodule_search_locations:
        return None
    for d in spec.submodule_search_locations:
        hip = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(hip):
            return ctypes.CDLL(hip, mode=ctypes.RTLD_GLOBAL)
    return None


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    _share_torch_hip_runtime()
    if not os.path.exists(path):
        raise RuntimeError(
            f"libshs_gpu.so not found at {path}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the raster path)")
    lib = ctypes.CDLL(path)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_LIB = None


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        _LIB = load()
    return _LIB
