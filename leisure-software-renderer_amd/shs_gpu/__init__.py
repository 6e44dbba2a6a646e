"""shs_gpu -- Python mirror of the shs_renderer legacy draw-call API over libshs_gpu.so.

The reference drives its hot path from C++ (`RendererSystem::process` -> `draw_triangle_tile`,
cpp-folders/src/hello-3d-primitives/hello_pipeline_blinn_phong_shading.cpp:244-313).  This module
is the thin host layer the tests and bench use: it owns a context (`shs_create`), uploads meshes
once (`shs_mesh_upload_soup`, the ModelGeometry soup), enqueues frames (`shs_render_legacy`) and
resolves framebuffers into the reference layouts (`shs_resolve`).  Every call goes through the C ABI
into the gfx950 kernels; there is no CPU path here.
"""
import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _abi
from ._abi import (FRAME_PREQUANT, FRAME_PRESENT, SHADING_BLINN_PHONG, SHADING_DEPTH_VIS, SHADING_FLAT, SHADING_GOOCH,
                   SHADING_GOURAUD, SHADING_NAMES, SHADING_NORMAL_VIS, SHADING_OREN_NAYAR, SHADING_PHONG, SHADING_TEXTURED,
                   SHADING_TOON, FrameDesc, LegacyDraw, RasterStats)

__all__ = [
    "ShsError", "Context", "Frame", "Draw", "RtFrame", "RtDraw", "RtPcss", "RtPbrDraw", "RtPbr", "RtSky", "RtSkyboxIblDraw", "RtIblPhongDraw", "RtWaterDraw", "RtWater", "SHADING_FLAT", "SHADING_GOURAUD", "SHADING_PHONG",
    "SHADING_BLINN_PHONG", "SHADING_TOON", "SHADING_GOOCH", "SHADING_OREN_NAYAR", "SHADING_NORMAL_VIS",
    "SHADING_DEPTH_VIS", "SHADING_TEXTURED", "SHADING_NAMES", "FRAME_PREQUANT", "lib",
]

lib = _abi.lib


class ShsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"shs_gpu error {code}: {msg}")
        self.code = code


def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


@dataclass
class Draw:
    """One object of the legacy scene loop: the reference's `Uniforms` + mesh + shading model."""
    mesh: object                 # Mesh (positions/normals float32 [n,9]) or an uploaded mesh id
    shading: int
    mvp: np.ndarray              # float32[16], column-major (glm::mat4 storage)
    model: np.ndarray            # float32[16] (Flat: Uniforms::mv)
    light_dir: np.ndarray        # float32[3]  (Flat: light_dir_view)
    camera_pos: np.ndarray       # float32[3]
    color: tuple = (60, 100, 200, 255)
    # SHADING_TEXTURED: an uploaded texture id (0: no texture, Uniforms::color) or an object with .rgba [h, w, 4].
    # A frame or batch with any draw's albedo_tex set goes through shs_render_legacy_batch_tex, the call that
    # takes the textured model; with none set it is shs_render_legacy[_batch], which takes models 0..8 as ever.
    albedo_tex: object = None


@dataclass
class Frame:
    width: int
    height: int
    ref_tile: tuple = (80, 80)   # TILE_SIZE_X/Y of the legacy pipelines
    shard_rank: int = 0
    shard_count: int = 1
    clear_color: tuple = (0, 0, 0, 255)
    prequant: bool = False
    present: bool = False             # SHS_FRAME_PRESENT: also write the SDL staging
    debug_flags: int = 0         # timing experiments only (bits 8+, wrong images)

    def desc(self) -> FrameDesc:
        d = FrameDesc()
        d.width, d.height = self.width, self.height
        d.ref_tile_w, d.ref_tile_h = self.ref_tile
        d.shard_rank, d.shard_count = self.shard_rank, self.shard_count
        d.flags = (FRAME_PREQUANT if self.prequant else 0) | (FRAME_PRESENT if self.present else 0) | \
                  (int(self.debug_flags) & ~0xff)
        for i in range(4):
            d.clear_color[i] = self.clear_color[i]
        return d


@dataclass
class RtDraw:
    """One object of the Canvas render-target passes (shs_rt_draw): the per-object part of
    hello_shadow_mapping.cpp's Uniforms.  The shadow pass reads mesh and model only."""
    mesh: object                 # Mesh (positions / normals [n, 9], optional uvs [n, 6]) or an uploaded soup id
    model: np.ndarray            # float32[16], column-major
    mvp: np.ndarray = None
    prev_mvp: np.ndarray = None
    base_color: tuple = (200, 200, 200, 255)
    albedo_tex: object = None    # an uploaded texture id, an object with .rgba [h, w, 4], or None (base_color)


@dataclass
class RtFrame:
    """The camera pass's frame (shs_rt_frame); the defaults are the demo's constants."""
    width: int
    height: int
    view: np.ndarray
    light_vp: np.ndarray
    light_dir_world: tuple
    camera_pos: tuple
    ref_tile: tuple = (80, 80)
    clear_color: tuple = (20, 20, 25, 255)
    bias_base: float = 0.0025
    bias_slope: float = 0.01
    max_velocity_px: float = 22.0
    use_shadow: bool = True
    pcf: bool = True
    prequant: bool = False
    shading: int = 0             # 0: fragment_shader_full, 1: fragment_shader_softshadow (PCSS; Context.rt_set_pcss),
                                 # 2: fragment_shader_pbr (Context.rt_render_pbr only),
                                 # 3: hello_pbr_light_shafts.cpp's fragment_shader_pbr, PBR under PCSS (Context.rt_render_pbr_soft only)
                                 # 4: hello_ibl_skybox.cpp's sky-lit fragment_shader_full (Context.rt_render_skybox_ibl only)
                                 # 5: hello_water.cpp's atmosphere and water shaders, chosen per draw (Context.rt_render_water only)
                                 # 6: hello_multi_pass.cpp's blinn_phong_fragment_shader, 7: hello_glowing_star.cpp's
                                 #    star_fragment_shader, both behind the unclipped raster (Context.rt_render_motion only)
                                 # 8: hello_per_object_motion_blur.cpp's velocity_fragment_shader, 9: hello_depth_of_field.cpp's
                                 #    and 10: hello_ping_pong.cpp's Blinn-Phong shader (Context.rt_render_plain only; the depth
                                 #    plane is then in screen rows)
                                 # 11: hello_ibl_skybox_optimized.cpp's / hello_ibl_skybox_xsimd.cpp's fragment_shader_full, Blinn-Phong
                                 #    with a per-draw shininess plus the IBL of rt_set_ibl (Context.rt_render_ibl_phong only)


@dataclass
class RtPcss:
    """The PCSS constants of RtFrame.shading 1 (shs_rt_pcss); the defaults are hello_shadow_mapping_soft.cpp's."""
    light_uv_radius: float = 0.0035
    search_radius_texels: float = 18.0
    min_filter_texels: float = 1.0
    max_filter_texels: float = 28.0
    epsilon: float = 1e-5
    blocker_samples: int = 12
    pcf_samples: int = 24


@dataclass
class RtPbrDraw:
    """hello_pbr.cpp's per-object uniforms beside an RtDraw (shs_rt_pbr_draw); the defaults are MaterialPBR's and
    Uniforms'.  normal_mat: float32[9], column-major mat3, as the demo supplies it (None: mat3(1))."""
    normal_mat: np.ndarray = None
    metallic: float = 0.0
    roughness: float = 0.5
    ao: float = 1.0
    ibl_diffuse_intensity: float = 0.30
    ibl_specular_intensity: float = 0.35
    ibl_reflection_strength: float = 1.00


@dataclass
class RtPbr:
    """The constants of fragment_shader_pbr (shs_rt_pbr); the defaults are hello_pbr.cpp's."""
    exposure: float = 1.75
    min_roughness: float = 0.04
    direct_intensity: float = 3.0


@dataclass
class RtSkyboxIblDraw:
    """hello_ibl_skybox.cpp's per-object knobs beside an RtDraw (shs_rt_skybox_ibl_draw); the defaults are Uniforms'."""
    ibl_ambient: float = 0.25
    ibl_refl: float = 0.35
    ibl_f0: float = 0.04
    ibl_refl_mix: float = 1.0


@dataclass
class RtIblPhongDraw:
    """hello_ibl_skybox_optimized.cpp's / hello_ibl_skybox_xsimd.cpp's per-object knobs beside an RtDraw
    (shs_rt_ibl_phong_draw); the defaults are Uniforms'."""
    ibl_ambient: float = 0.30
    ibl_refl: float = 0.35
    ibl_f0: float = 0.04
    ibl_refl_mix: float = 1.0
    shininess: float = 64.0


@dataclass
class RtWaterDraw:
    """Which of hello_water.cpp's two fragment shaders an RtDraw runs (shs_rt_water_draw): fragment_shader_water for the
    water surface, the atmosphere fragment_shader_full for everything else."""
    surface: bool = False


@dataclass
class RtWater:
    """The frame's part of hello_water.cpp's Uniforms (shs_rt_water).  reflection_vp: float32[16], the mirrored camera's
    proj * view, column-major (None: identity, the Uniforms default); reflection: read the context's reflection canvas
    (Context.rt_keep_reflection / rt_set_reflection), else the water reflects the sky colour."""
    reflection_vp: np.ndarray = None
    time_sec: float = 0.0
    reflection: bool = False


@dataclass
class RtSky:
    """The background of the camera passes (shs_rt_sky): a legacy sky model of shs_renderer.hpp and the camera of
    skybox_background_pass; the defaults are hello_pbr.cpp's (AnalyticSky's default sun, SKY_EXPOSURE)."""
    model: int = _abi.RT_SKY_ANALYTIC
    encode: int = _abi.RT_SKY_ENCODE_REINHARD
    sun_dir: tuple = (0.4668, -0.3487, 0.8127)
    intensity: float = 1.0
    face_tex: tuple = ()         # cubemap: +X -X +Y -Y +Z -Z, each an uploaded texture id or an object with .rgba [h, w, 4]
    cam_forward: tuple = (0.0, 0.0, 1.0)
    cam_right: tuple = (1.0, 0.0, 0.0)
    cam_up: tuple = (0.0, 1.0, 0.0)
    fov_degrees: float = 60.0
    exposure: float = 1.85


class Context:
    """A libshs_gpu context bound to one HIP device (one host thread at a time)."""

    def __init__(self, device: int = 0):
        self._lib = lib()
        h = ctypes.c_void_p()
        rc = self._lib.shs_create(device, ctypes.byref(h))
        if rc != 0:
            raise ShsError(rc, f"shs_create(device={device}) failed (no gfx950 device?)")
        self._h = h
        self._meshes = {}
        self._frame = None
        self._lib_frame = None
        self._shadow_size = None
        self._rt_size = None
        self._rt_shadow_size = None

    def _check(self, rc):
        if rc != 0:
            raise ShsError(rc, self._lib.shs_last_error(self._h).decode(errors="replace"))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.shs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- geometry -----------------------------------------------------------------------------
    def upload_mesh(self, mesh) -> int:
        key = id(mesh)
        if key in self._meshes:
            return self._meshes[key][0]
        mid = self.upload_soup(mesh.positions, mesh.normals, getattr(mesh, "uvs", None))
        self._meshes[key] = (mid, mesh)
        return mid

    def upload_soup(self, positions, normals, uvs=None) -> int:
        """shs_mesh_upload_soup[_uv]: positions / normals float32 [n, 9] and, for SHADING_TEXTURED, uvs [n, 6]
        (ModelGeometry::uvs; None: the model reads vec2(0) per corner) -> mesh id."""
        pos = np.ascontiguousarray(positions, dtype=np.float32)
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        assert pos.shape == nrm.shape and pos.shape[-1] == 9
        mid = ctypes.c_int32()
        if uvs is None:
            self._check(self._lib.shs_mesh_upload_soup(self._h, _fptr(pos), _fptr(nrm), pos.shape[0], ctypes.byref(mid)))
        else:
            uv = np.ascontiguousarray(uvs, dtype=np.float32)
            assert uv.shape == (pos.shape[0], 6)
            self._check(self._lib.shs_mesh_upload_soup_uv(self._h, _fptr(pos), _fptr(nrm), _fptr(uv), pos.shape[0],
                                                          ctypes.byref(mid)))
        return mid.value

    # -- frames -------------------------------------------------------------------------------
    def _draw_array(self, draws):
        arr = (LegacyDraw * max(len(draws), 1))()
        for i, d in enumerate(draws):
            a = arr[i]
            a.mesh_id = d.mesh if isinstance(d.mesh, int) else self.upload_mesh(d.mesh)
            a.shading = int(d.shading)
            for k in range(16):
                a.mvp[k] = float(d.mvp[k])
                a.model[k] = float(d.model[k])
            for k in range(3):
                a.light_dir[k] = float(d.light_dir[k])
                a.camera_pos[k] = float(d.camera_pos[k])
            for k in range(4):
                a.color[k] = int(d.color[k])
        arr.albedo_tex = self._tex_array(draws)   # (travels with the draws: the parallel array of ids, or None)
        return arr

    def _tex_array(self, draws):
        """The draws' albedo_tex as shs_render_legacy_batch_tex's parallel id array; None when no draw has one."""
        texs = [getattr(d, "albedo_tex", None) for d in draws]
        if all(t is None for t in texs):
            return None
        ids = (ctypes.c_int32 * max(len(draws), 1))()
        for i, t in enumerate(texs):
            ids[i] = 0 if t is None else (int(t) if isinstance(t, (int, np.integer)) else self.upload_texture(t))
        return ids

    def prepare(self, frame: Frame, draws):
        """Build the ctypes frame/draw arrays once (re-used by render_prepared in timed loops)."""
        return frame, frame.desc(), self._draw_array(draws), len(draws)

    def render_prepared(self, prepared):
        frame, desc, arr, n = prepared
        tex = getattr(arr, "albedo_tex", None)
        if tex is None:
            self._check(self._lib.shs_render_legacy(self._h, ctypes.byref(desc), arr, n))
        else:
            self._check(self._lib.shs_render_legacy_batch_tex(self._h, ctypes.byref(desc), arr, tex, n, 1))
        self._frame = frame

    def render(self, frame: Frame, draws):
        self.render_prepared(self.prepare(frame, draws))

    def prepare_batch(self, frame: Frame, frames_draws):
        """frames_draws: one draw list per frame (equal lengths and triangle counts) -> prepared batch."""
        n = len(frames_draws[0])
        assert all(len(d) == n for d in frames_draws), "every frame of a batch has the same number of draws"
        flat = [d for fd in frames_draws for d in fd]
        return frame, frame.desc(), self._draw_array(flat), n, len(frames_draws)

    def render_batch_prepared(self, prepared):
        frame, desc, arr, n, n_frames = prepared
        tex = getattr(arr, "albedo_tex", None)
        if tex is None:
            self._check(self._lib.shs_render_legacy_batch(self._h, ctypes.byref(desc), arr, n, n_frames))
        else:
            self._check(self._lib.shs_render_legacy_batch_tex(self._h, ctypes.byref(desc), arr, tex, n, n_frames))
        self._frame = frame
        self._n_frames = n_frames

    def render_batch(self, frame: Frame, frames_draws):
        """shs_render_legacy_batch: one k_setup + k_raster pair renders every frame of the batch."""
        self.render_batch_prepared(self.prepare_batch(frame, frames_draws))

    def legacy_sample_nearest(self, tex, uv):
        """shs_legacy_sample_nearest: sample_nearest of texture `tex` (an id, or an object with .rgba) at uv [n, 2]
        through the function the rasters call -> rgba uint8 [n, 4] (alpha 255)."""
        tid = int(tex) if isinstance(tex, (int, np.integer)) else self.upload_texture(tex)
        c = np.ascontiguousarray(np.asarray(uv, np.float32).reshape(-1, 2))
        rgba = np.zeros((c.shape[0], 4), np.uint8)
        self._check(self._lib.shs_legacy_sample_nearest(self._h, tid, c.shape[0], _fptr(c), rgba.ctypes.data_as(ctypes.c_void_p)))
        return rgba

    def release_texture(self, tex_id):
        """shs_texture_release (a legacy batch in flight that samples it is finished first)."""
        self._check(self._lib.shs_texture_release(self._h, int(tex_id)))

    def legacy_shade_samples(self, shading, light_dir, camera_pos, color, normal_sum, world_pos, clip_z):
        """shs_legacy_shade_samples: the legacy fragment shader `shading` (any model but Flat and Gouraud) for n
        samples of interpolated varyings -- normal_sum [n, 3] (before draw_triangle_tile's normalise), world_pos
        [n, 3], clip_z [n] -- under the uniforms light_dir, camera_pos, color
        -> (rgba uint8 [n, 4], pre-truncation floats float32 [n, 4])."""
        ns = np.ascontiguousarray(np.asarray(normal_sum, np.float32).reshape(-1, 3))
        wp = np.ascontiguousarray(np.asarray(world_pos, np.float32).reshape(-1, 3))
        cz = np.ascontiguousarray(np.asarray(clip_z, np.float32).reshape(-1))
        n = ns.shape[0]
        assert wp.shape[0] == n and cz.shape[0] == n
        u = LegacyDraw()
        u.mesh_id, u.shading = -1, int(shading)
        for k in range(3):
            u.light_dir[k] = float(light_dir[k])
            u.camera_pos[k] = float(camera_pos[k])
        for k in range(4):
            u.color[k] = int(color[k])
        rgba = np.zeros((n, 4), np.uint8)
        pq = np.zeros((n, 4), np.float32)
        self._check(self._lib.shs_legacy_shade_samples(self._h, ctypes.byref(u), n, _fptr(ns), _fptr(wp), _fptr(cz),
                                                       rgba.ctypes.data_as(ctypes.c_void_p),
                                                       pq.ctypes.data_as(ctypes.c_void_p)))
        return rgba, pq

    def resolve_frame(self, index: int):
        f = self._frame
        color = np.empty((f.height, f.width, 4), dtype=np.uint8)
        depth = np.empty((f.height, f.width), dtype=np.float32)
        self._check(self._lib.shs_resolve_frame(self._h, int(index), color.ctypes.data_as(ctypes.c_void_p),
                                                depth.ctypes.data_as(ctypes.c_void_p)))
        return color, depth

    def synchronize(self):
        self._check(self._lib.shs_synchronize(self._h))

    def resolve(self):
        f = self._frame
        color = np.empty((f.height, f.width, 4), dtype=np.uint8)
        depth = np.empty((f.height, f.width), dtype=np.float32)
        self._check(self._lib.shs_resolve(self._h, color.ctypes.data_as(ctypes.c_void_p),
                                          depth.ctypes.data_as(ctypes.c_void_p)))
        return color, depth

    def present_device(self, index: int = 0) -> int:
        """Device address of frame `index`'s SDL staging (SHS_FRAME_PRESENT); a batch's frames are
        contiguous, W * H * 4 bytes apart."""
        p = ctypes.c_void_p()
        self._check(self._lib.shs_present_device(self._h, int(index), ctypes.byref(p)))
        return p.value

    def resolve_present(self, index: int = 0, pitch: int = 0):
        """The SDL staging of frame `index` (Canvas::copy_to_SDLSurface): uint8 [H, W, 4], rows top-down.
        pitch > W*4 pads rows as an SDL surface would (returned array [H, pitch] bytes)."""
        f = self._frame
        pitch = pitch or f.width * 4
        out = np.zeros((f.height, pitch), dtype=np.uint8)
        self._check(self._lib.shs_resolve_present(self._h, int(index), out.ctypes.data_as(ctypes.c_void_p), pitch))
        return out if pitch != f.width * 4 else out.reshape(f.height, f.width, 4)

    def resolve_prequant(self, index: int = 0):
        """Pre-truncation shader floats of frame `index` of the last batch (SHS_FRAME_PREQUANT)."""
        f = self._frame
        pq = np.empty((f.height, f.width, 4), dtype=np.float32)
        self._check(self._lib.shs_resolve_prequant_frame(self._h, int(index), pq.ctypes.data_as(ctypes.c_void_p)))
        return pq

    def device_framebuffers(self):
        c, d = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.shs_device_framebuffers(self._h, ctypes.byref(c), ctypes.byref(d)))
        return c.value, d.value

    def stats(self) -> dict:
        s = RasterStats()
        self._check(self._lib.shs_get_stats(self._h, ctypes.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in RasterStats._fields_}

    def enable_timing(self, on=True):
        self._check(self._lib.shs_enable_timing(self._h, 1 if on else 0))

    def kernel_ms(self):
        ms = (ctypes.c_float * 4)()
        self._check(self._lib.shs_last_kernel_ms(self._h, ms))
        return {"setup": ms[0], "raster": ms[3]}

    def timing_reset(self):
        self._check(self._lib.shs_timing_reset(self._h))

    def timing_read(self):
        """-> (frames, {kernel: mean ms}) over every frame since timing_reset()."""
        s = (ctypes.c_double * 4)()
        n = ctypes.c_int64()
        self._check(self._lib.shs_timing_read(self._h, s, ctypes.byref(n)))
        k = max(n.value, 1)
        return n.value, {"setup": s[0] / k, "raster": s[3] / k}

    # shs_dev::TriHot (64 B): word = draw | flags << 29
    TRIREC_DTYPE = np.dtype([
        ("ax", "<f4"), ("ay", "<f4"), ("v0x", "<f4"), ("v0y", "<f4"), ("v1x", "<f4"), ("v1y", "<f4"),
        ("d00", "<f4"), ("d01", "<f4"), ("d11", "<f4"), ("denom", "<f4"), ("z0", "<f4"), ("z1", "<f4"),
        ("z2", "<f4"), ("word", "<u4"), ("gbx", "<u4"), ("gby", "<u4")])

    def debug_records(self):
        """The last frame's per-triangle raster records (structured numpy array)."""
        n = ctypes.c_int64()
        self._check(self._lib.shs_debug_records(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=self.TRIREC_DTYPE)
        self._check(self._lib.shs_debug_records(self._h, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        return out

    def set_raster_mode(self, mode: int):
        """0 auto, 1 scan (no bins), 2 bins."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_RASTER_MODE, int(mode)))

    def set_raster_loop(self, loop: int):
        """Legacy raster inner loop: 1 (candidate, pixel) pair tasks (default), 0 per-pixel candidate loop."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_RASTER_LOOP, int(loop)))

    def set_timeline(self, enable: bool, shadow: bool = False):
        """Workgroup timelines of the frames that follow; shadow: the library shadow pass's raster
        (lib_debug_timeline) instead of the camera pass's."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_TIMELINE, (2 if shadow else 1) if enable else 0))

    # -- after the path: PassTonemap + present staging ------------------------------------------
    def tonemap(self, exposure: float = 1.0, gamma: float = 2.2, ldr: bool = True, present: bool = True):
        """PassTonemap (pass_tonemap.hpp:36-83) over the last camera pass's HDR target into the
        RT_ColorLDR layout and / or the SDL staging of upload_ldr_to_rgba8 (one launch)."""
        d = _abi.TonemapDescC()
        d.exposure, d.gamma = float(exposure), float(gamma)
        d.flags = (_abi.TONEMAP_LDR if ldr else 0) | (_abi.TONEMAP_PRESENT if present else 0)
        self._check(self._lib.shs_tonemap(self._h, ctypes.byref(d)))
        self._tonemap_flags = d.flags

    def fuse_tonemap(self, exposure: float = 1.0, gamma: float = 2.2, ldr: bool = True, present: bool = True,
                     enable: bool = True):
        """Fused PassTonemap: later camera passes also write the tonemap targets from their shading
        kernel (the same bytes as tonemap() after the pass); enable=False turns it off."""
        if not enable:
            self._check(self._lib.shs_lib_fuse_tonemap(self._h, None))
            return
        d = _abi.TonemapDescC()
        d.exposure, d.gamma = float(exposure), float(gamma)
        d.flags = (_abi.TONEMAP_LDR if ldr else 0) | (_abi.TONEMAP_PRESENT if present else 0)
        self._check(self._lib.shs_lib_fuse_tonemap(self._h, ctypes.byref(d)))
        self._tonemap_flags = d.flags

    def _sky_desc(self, sky):
        faces = sky.faces if sky.model == _abi.SKY_CUBEMAP and sky.faces is not None else None
        return sky.desc(None if faces is None else [self.upload_texture(t) for t in faces])

    def set_sky(self, sky=None):
        """shs_lib_set_sky: later camera passes paint lib_path.LibSky `sky` behind the meshes (sticky; a moving
        camera sets it per frame); None: back to the gradient / clear_hdr."""
        if sky is None or sky.model == _abi.SKY_NONE:
            self._check(self._lib.shs_lib_set_sky(self._h, None))
            return
        d = self._sky_desc(sky)
        self._check(self._lib.shs_lib_set_sky(self._h, ctypes.byref(d)))

    def sky_sample(self, sky, dirs):
        """shs_sky_sample: ISkyModel::sample of `sky` for dirs float32 [n, 3] -> rgb float32 [n, 3]."""
        dirs = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3))
        rgb = np.zeros_like(dirs)
        d = self._sky_desc(sky)
        fp = ctypes.POINTER(ctypes.c_float)
        self._check(self._lib.shs_sky_sample(self._h, ctypes.byref(d), dirs.ctypes.data_as(fp), dirs.shape[0],
                                             rgb.ctypes.data_as(fp)))
        return rgb

    def resolve_ldr(self):
        """-> (ldr uint8 [H, W, 4] rows y up or None, present uint8 [H, W, 4] rows top-down or None)."""
        f = self._lib_frame
        flags = getattr(self, "_tonemap_flags", 0)
        ldr = np.empty((f.height, f.width, 4), np.uint8) if flags & _abi.TONEMAP_LDR else None
        pre = np.empty((f.height, f.width, 4), np.uint8) if flags & _abi.TONEMAP_PRESENT else None
        self._check(self._lib.shs_resolve_ldr(self._h, None if ldr is None else ldr.ctypes.data_as(ctypes.c_void_p),
                                              None if pre is None else pre.ctypes.data_as(ctypes.c_void_p)))
        return ldr, pre

    def light_shafts(self, viewproj, cam_pos, sun_dir_ws, enable=True, steps=48, density=0.8, weight=0.9, decay=0.95,
                     use_depth=True):
        """PassLightShafts (pass_light_shafts.hpp:44-215) on the last tonemap's RT_ColorLDR in place (and
        its present staging), with the camera pass's depth plane when it has one and use_depth
        (defaults: LightShaftsPassParams).  viewproj: column-major float[16], as LibDraw.viewproj.
        resolve_ldr() then returns the shafted bytes."""
        d = _abi.LightShaftsDescC()
        d.enable, d.steps = 1 if enable else 0, int(steps)
        d.density, d.weight, d.decay = float(density), float(weight), float(decay)
        d.cam_pos[:] = [float(v) for v in cam_pos]
        d.sun_dir_ws[:] = [float(v) for v in sun_dir_ws]
        d.viewproj[:] = [float(v) for v in np.asarray(viewproj, np.float32).reshape(16)]
        d.flags = 0 if use_depth else _abi.LIGHT_SHAFTS_NO_DEPTH
        self._check(self._lib.shs_light_shafts(self._h, ctypes.byref(d)))

    @staticmethod
    def light_shafts_sun_uv(viewproj, cam_pos, sun_dir_ws):
        """PassLightShafts' sun projection (pass_light_shafts.hpp:78-92) -> (sun_uv float32[2], valid)."""
        fp = ctypes.POINTER(ctypes.c_float)
        a = [np.ascontiguousarray(np.asarray(v, np.float32).reshape(n)) for v, n in ((cam_pos, 3), (sun_dir_ws, 3), (viewproj, 16))]
        uv = np.zeros(2, np.float32)
        valid = ctypes.c_int32(0)
        rc = lib().shs_light_shafts_sun_uv(*[v.ctypes.data_as(fp) for v in a], uv.ctypes.data_as(fp), ctypes.byref(valid))
        if rc != 0:
            raise ShsError(rc, "shs_light_shafts_sun_uv")
        return uv, bool(valid.value)

    def motion_blur(self, enable=True, samples=10, strength=1.0, max_velocity_px=20.0, min_velocity_px=0.25,
                    depth_reject=0.08, dt=1.0 / 60.0, present=True):
        """PassMotionBlur (pass_motion_blur.hpp:38-170) over the last tonemap's RT_ColorLDR with the
        camera pass's depth / motion planes (defaults: MotionBlurPassParams)."""
        d = _abi.MotionBlurDescC()
        d.enable, d.samples = 1 if enable else 0, int(samples)
        d.strength, d.max_velocity_px, d.min_velocity_px = float(strength), float(max_velocity_px), float(min_velocity_px)
        d.depth_reject, d.dt = float(depth_reject), float(dt)
        d.flags = _abi.MOTION_BLUR_PRESENT if present else 0
        self._check(self._lib.shs_motion_blur(self._h, ctypes.byref(d)))
        self._mb_present = bool(present)

    def resolve_motion_blur(self):
        """-> (blurred RT_ColorLDR uint8 [H, W, 4] rows y up, present staging or None)."""
        f = self._lib_frame
        ldr = np.empty((f.height, f.width, 4), np.uint8)
        pre = np.empty((f.height, f.width, 4), np.uint8) if getattr(self, "_mb_present", False) else None
        self._check(self._lib.shs_resolve_motion_blur(self._h, ldr.ctypes.data_as(ctypes.c_void_p),
                                                      None if pre is None else pre.ctypes.data_as(ctypes.c_void_p)))
        return ldr, pre

    def occlusion_pass(self, width, height, view, view_proj, objects, frustum_visible, depth_epsilon=1e-4,
                       enable=True):
        """culling_sw::run_software_occlusion_pass (culling_software.hpp:229-331).  objects: sequence of
        (LibMesh with indices, model float[16], aabb_min[3], aabb_max[3]) -> (occluded uint8 [n],
        visible uint32 [k] in visit order, depth float32 [height, width])."""
        n = len(objects)
        # shs_occluder records (int32 mesh_id, float model[16], aabb_min[3], aabb_max[3]) built in numpy
        arr = np.zeros((max(n, 1), ctypes.sizeof(_abi.OccluderC) // 4), np.float32)
        if n:
            arr[:n, 0].view(np.int32)[:] = [self.upload_lib_mesh(o[0]) for o in objects]
            arr[:n, 1:17] = np.asarray([o[1] for o in objects], np.float32).reshape(n, 16)
            arr[:n, 17:20] = np.asarray([o[2] for o in objects], np.float32).reshape(n, 3)
            arr[:n, 20:23] = np.asarray([o[3] for o in objects], np.float32).reshape(n, 3)
        d = _abi.OcclusionDescC()
        d.width, d.height = int(width), int(height)
        for k in range(16):
            d.view[k], d.view_proj[k] = float(view[k]), float(view_proj[k])
        d.depth_epsilon, d.enable = float(depth_epsilon), 1 if enable else 0
        fv = np.ascontiguousarray(frustum_visible, dtype=np.uint32)
        occ = np.zeros(max(n, 1), np.uint8)
        vis = np.zeros(max(fv.size, 1), np.uint32)
        nv = ctypes.c_int32()
        depth = np.zeros((height, width), np.float32)
        self._check(self._lib.shs_occlusion_pass(self._h, ctypes.byref(d), arr.ctypes.data_as(ctypes.POINTER(_abi.OccluderC)), n,
                                                 fv.ctypes.data_as(ctypes.c_void_p),
                                                 fv.size, occ.ctypes.data_as(ctypes.c_void_p),
                                                 vis.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nv),
                                                 depth.ctypes.data_as(ctypes.c_void_p)))
        return occ[:n], vis[:nv.value], depth

    def debug_draw_meshes(self, width, height, view_proj, camera_pos, light_dir_ws, meshes, rgba=None, depth=None,
                          tri_lit=False):
        """debug_draw::draw_mesh_blinn_phong_transformed (sw_render/debug_draw.hpp:147-203) over meshes =
        sequence of (LibMesh with indices, model float[16], base_color[3]), in order.  rgba uint8
        [height, width, 4] (RT_ColorLDR, y * W + x) and depth float32 [height, width] are drawn into in
        place (defaults: cleared to 0 / 1.0).  Returns (rgba, depth) or, with tri_lit, (rgba, depth,
        float32 [n_tris, 4] lit rgb + area-test flag)."""
        rgba = np.zeros((height, width, 4), np.uint8) if rgba is None else rgba
        depth = np.ones((height, width), np.float32) if depth is None else depth
        assert rgba.shape == (height, width, 4) and rgba.dtype == np.uint8 and rgba.flags.c_contiguous
        assert depth.shape == (height, width) and depth.dtype == np.float32 and depth.flags.c_contiguous
        n = len(meshes)
        # shs_debug_mesh records (int32 mesh_id, float model[16], base_color[3]) built in numpy
        arr = np.zeros((max(n, 1), ctypes.sizeof(_abi.DebugMeshC) // 4), np.float32)
        n_tris = 0
        if n:
            arr[:n, 0].view(np.int32)[:] = [self.upload_lib_mesh(m[0]) for m in meshes]
            arr[:n, 1:17] = np.asarray([m[1] for m in meshes], np.float32).reshape(n, 16)
            arr[:n, 17:20] = np.asarray([m[2] for m in meshes], np.float32).reshape(n, 3)
            n_tris = sum(len(m[0].indices) // 3 for m in meshes)
        d = _abi.DebugDrawDescC()
        d.width, d.height = int(width), int(height)
        for k in range(16):
            d.view_proj[k] = float(view_proj[k])
        for k in range(3):
            d.camera_pos[k], d.light_dir_ws[k] = float(camera_pos[k]), float(light_dir_ws[k])
        lit = np.zeros((max(n_tris, 1), 4), np.float32) if tri_lit else None
        self._check(self._lib.shs_debug_draw_meshes(self._h, ctypes.byref(d), arr.ctypes.data_as(ctypes.POINTER(_abi.DebugMeshC)),
                                                    n, rgba.ctypes.data_as(ctypes.c_void_p),
                                                    depth.ctypes.data_as(ctypes.c_void_p),
                                                    None if lit is None else lit.ctypes.data_as(ctypes.c_void_p)))
        return (rgba, depth, lit[:n_tris]) if tri_lit else (rgba, depth)

    def debug_fill_triangles(self, width, height, screen, z, colors, rgba=None, depth=None):
        """debug_draw::draw_filled_triangle (debug_draw.hpp:60-109) for each triangle in order: screen
        float32 [n, 3, 2] points, z float32 [n, 3], colors uint8 [n, 4]."""
        rgba = np.zeros((height, width, 4), np.uint8) if rgba is None else rgba
        depth = np.ones((height, width), np.float32) if depth is None else depth
        assert rgba.shape == (height, width, 4) and rgba.dtype == np.uint8 and rgba.flags.c_contiguous
        assert depth.shape == (height, width) and depth.dtype == np.float32 and depth.flags.c_contiguous
        screen = np.asarray(screen, np.float32).reshape(-1, 6)
        n = screen.shape[0]
        rec = np.zeros((max(n, 1), ctypes.sizeof(_abi.DebugTriangleC) // 4), np.float32)
        rec[:n, 0:6] = screen
        rec[:n, 6:9] = np.asarray(z, np.float32).reshape(n, 3)
        rec[:n, 9].view(np.uint32)[:] = np.ascontiguousarray(colors, np.uint8).reshape(n, 4).view(np.uint32).reshape(n)
        self._check(self._lib.shs_debug_fill_triangles(self._h, int(width), int(height),
                                                       rec.ctypes.data_as(ctypes.POINTER(_abi.DebugTriangleC)), n,
                                                       rgba.ctypes.data_as(ctypes.c_void_p),
                                                       depth.ctypes.data_as(ctypes.c_void_p)))
        return rgba, depth

    CANVAS_DEVICE = 1

    def _on_torch_stream(self):
        """Device-tensor calls run on torch's current stream, so they are ordered after the torch work
        that wrote their inputs and before the torch work that reads their outputs (tensors allocated
        here, e.g. dst, belong to that stream too).  The context is re-pointed only when it is on
        another stream (shs_set_stream synchronises)."""
        import torch
        s = torch.cuda.current_stream().cuda_stream
        if self.stream != s:
            self.set_stream(s)

    def canvas_motion_blur(self, src, depth, velocity, curr_view, curr_proj, prev_view, prev_proj, samples=12,
                           strength=0.85, w_obj=1.0, w_cam=0.35, soft_knee=True, knee_px=18.0, max_px=22.0, dst=None):
        """combined_motion_blur_pass (hello_pbr.cpp:1128-1252).  Host arrays: src uint8 [H, W, 4], depth
        float32 [H, W] (view z), velocity float32 [H, W, 2] -> dst uint8 [H, W, 4].  torch CUDA tensors of
        the same shapes run on the device (asynchronous on the context stream)."""
        H, W = src.shape[:2]
        d = _abi.CanvasMotionBlurDescC()
        d.width, d.height = W, H
        for k in range(16):
            d.curr_view[k], d.curr_proj[k] = float(curr_view[k]), float(curr_proj[k])
            d.prev_view[k], d.prev_proj[k] = float(prev_view[k]), float(prev_proj[k])
        d.samples, d.strength, d.w_obj, d.w_cam = int(samples), float(strength), float(w_obj), float(w_cam)
        d.soft_knee, d.knee_px, d.max_px = 1 if soft_knee else 0, float(knee_px), float(max_px)
        dev = _is_device(src)
        if dev:
            self._on_torch_stream()
        if dst is None:
            dst = _empty_like(src)
        keep = (_host_c(src, np.uint8), _host_c(depth, np.float32), _host_c(velocity, np.float32), dst)
        self._check(self._lib.shs_canvas_motion_blur(self._h, ctypes.byref(d), *[_ptr(a) for a in keep],
                                                     self.CANVAS_DEVICE if dev else 0))
        return dst

    def canvas_gaussian_blur(self, src, horizontal, dst=None):
        """gaussian_blur_pass (hello_depth_of_field.cpp:175-251), one axis."""
        H, W = src.shape[:2]
        dev = _is_device(src)
        if dev:
            self._on_torch_stream()
        if dst is None:
            dst = _empty_like(src)
        src = _host_c(src, np.uint8)
        self._check(self._lib.shs_canvas_gaussian_blur(self._h, W, H, _ptr(src), _ptr(dst),
                                                       1 if horizontal else 0, self.CANVAS_DEVICE if dev else 0))
        return dst

    def canvas_dof(self, color, depth, iterations=3, radius=6, focus=None, range_=24.0, max_blur=0.6, blur=None):
        """The DoF step of hello_depth_of_field.cpp:786-812 on color (sharp in, composite out, in place)
        -> (color, blur, focus_depth)."""
        H, W = color.shape[:2]
        d = _abi.CanvasDofDescC()
        d.width, d.height, d.blur_iterations, d.autofocus_radius = W, H, int(iterations), int(radius)
        d.focus_x, d.focus_y = (W // 2, H // 2) if focus is None else focus
        d.range, d.max_blur = float(range_), float(max_blur)
        dev = _is_device(color)
        if dev:
            self._on_torch_stream()
        if blur is None:
            blur = _empty_like(color)
        f = ctypes.c_float()
        depth = _host_c(depth, np.float32)
        self._check(self._lib.shs_canvas_dof(self._h, ctypes.byref(d), _ptr(color), _ptr(depth),
                                             _ptr(blur), ctypes.byref(f), self.CANVAS_DEVICE if dev else 0))
        return color, blur, f.value

    # LightShaftParams (hello_pbr_light_shafts.cpp:189-218), the demo's values
    LIGHT_SHAFTS_DEFAULTS = dict(enable=True, steps=40, max_dist=110.0, min_dist=1.0, base_density=0.18, height_falloff=0.10,
                                 noise_scale=0.65, noise_strength=0.60, jitter_amount=1.0, ambient_strength=0.08,
                                 sigma_s=0.030, sigma_t=0.065, g=0.82, intensity=0.35, use_shadow=True, shadow_bias=0.0045,
                                 shadow_pcf_2x2=True)

    def canvas_light_shafts(self, src, depth, cam_pos, inv_view_proj, sun_dir_world, light_vp=None, shadow_map=None,
                            shadow_size=None, params=None, dst=None, prequant=False):
        """light_shafts_pass (hello_pbr_light_shafts.cpp:1525-1707).  Host arrays: src uint8 [H, W, 4], depth float32
        [H, W] (view z, FLT_MAX = empty) -> dst uint8 [H, W, 4]; torch CUDA tensors of the same shapes run on the
        device (asynchronous on the context stream; dst may be src).  shadow_map: float32 [h, w] of the same kind as
        src, or a device address with shadow_size = (w, h) (rt_device_shadow_map), or None (every step lit).
        params: LightShaftParams fields over LIGHT_SHAFTS_DEFAULTS.  prequant: also return float32 [H, W, 4], the
        colour * 255 before the byte truncation and the accumulated step count ((0, 0, 0, -1): a copied pixel)."""
        H, W = src.shape[:2]
        vals = dict(self.LIGHT_SHAFTS_DEFAULTS)
        unknown = set(params or ()) - set(vals)
        if unknown:
            raise TypeError(f"canvas_light_shafts: unknown parameters {sorted(unknown)}")
        vals.update(params or {})
        d = _abi.CanvasLightShaftsDescC()
        d.width, d.height = W, H
        for k in range(3):
            d.cam_pos[k], d.sun_dir_world[k] = float(cam_pos[k]), float(sun_dir_world[k])
        lvp = np.zeros(16, np.float32) if light_vp is None else np.asarray(light_vp, np.float32).reshape(16)
        ivp = np.asarray(inv_view_proj, np.float32).reshape(16)
        for k in range(16):
            d.inv_view_proj[k], d.light_vp[k] = float(ivp[k]), float(lvp[k])
        for name, ctype in _abi.CanvasLightShaftsDescC._fields_[8:]:
            setattr(d, name, int(vals[name]) if ctype is ctypes.c_int32 else float(vals[name]))
        dev = _is_device(src)
        if dev:
            self._on_torch_stream()
        if dst is None:
            dst = _empty_like(src)
        src, depth = _host_c(src, np.uint8), _host_c(depth, np.float32)
        map_ptr = None
        if isinstance(shadow_map, (int, np.integer)):
            if not dev:
                raise ValueError("canvas_light_shafts: a device shadow map goes with device buffers")
            d.shadow_w, d.shadow_h = shadow_size
            map_ptr = ctypes.c_void_p(int(shadow_map))
        elif shadow_map is not None:
            if _is_device(shadow_map) != dev:
                raise ValueError("canvas_light_shafts: shadow_map must live where src does")
            shadow_map = _host_c(shadow_map, np.float32)
            d.shadow_h, d.shadow_w = shadow_map.shape
            map_ptr = _ptr(shadow_map)
        pq = None
        if prequant:
            if dev:
                import torch
                pq = torch.empty((H, W, 4), dtype=torch.float32, device=src.device)
            else:
                pq = np.empty((H, W, 4), np.float32)
        self._check(self._lib.shs_canvas_light_shafts(self._h, ctypes.byref(d), _ptr(src), _ptr(depth), map_ptr, _ptr(dst),
                                                      None if pq is None else _ptr(pq), self.CANVAS_DEVICE if dev else 0))
        return (dst, pq) if prequant else dst

    # -- Canvas-API post passes (hello_multi_pass.cpp, hello_glowing_star.cpp) --------------------
    # The demos' constants (hello_multi_pass.cpp:66-100; hello_glowing_star.cpp:62-90 where it says so); a frame
    # method's per-pass dicts override them.  dof and motion_blur are canvas_dof's / canvas_motion_blur's arguments.
    FX_DEFAULTS = {
        "velocity_blur": dict(samples=12, strength=1.0),
        "fog": dict(fog_color=(28, 30, 38, 255), fog_start=20.0, fog_end=80.0, fog_power=1.25),
        "outline": dict(radius=1, threshold=0.75, strength=0.15),
        "fxaa": dict(reduce_min=1.0 / 128.0, reduce_mul=1.0 / 8.0, span_max=8.0),
        "spec_bright": dict(threshold=0.139, intensity=13.25),                                       # glowing star
        "lens_flare": dict(intensity=0.55, halo_intensity=0.35, chroma_shift_px=0.8, ghost_scales=(0.55, 0.85, 1.25)),
        "dof": dict(iterations=4, radius=6, focus=None, range_=34.0, max_blur=0.75),
        "motion_blur": dict(curr_view=None, curr_proj=None, prev_view=None, prev_proj=None, samples=12, strength=0.85,
                            w_obj=1.0, w_cam=0.35, soft_knee=True, knee_px=18.0, max_px=22.0),
        # hello_per_object_motion_blur.cpp:56-62; velocity_scale is the host's clampf(target_dt / dt, 0.25, 4), 1 at 60 Hz;
        # depth_rows 1: the depth plane is in screen rows, as rt_render_plain leaves it
        "object_blur": dict(multiplier=1.85, velocity_scale=1.0, min_vel2=0.25, max_samples=20, depth_eps=0.15, depth_rows=1),
    }
    _FX_DESCS = {"velocity_blur": _abi.CanvasVelocityBlurDescC, "fog": _abi.CanvasFogDescC, "outline": _abi.CanvasOutlineDescC,
                 "fxaa": _abi.CanvasFxaaDescC, "spec_bright": _abi.CanvasSpecBrightDescC, "lens_flare": _abi.CanvasLensFlareDescC,
                 "dof": _abi.CanvasDofDescC, "motion_blur": _abi.CanvasMotionBlurDescC, "object_blur": _abi.CanvasObjectBlurDescC}

    @classmethod
    def fx_desc(cls, kind, W, H, params=None, into=None):
        """The C desc of one post pass (kind: a key of FX_DEFAULTS) at W x H from FX_DEFAULTS and params; into: a desc
        to fill (a frame desc's member)."""
        vals = dict(cls.FX_DEFAULTS[kind])
        unknown = set(params or ()) - set(vals)
        if unknown:
            raise TypeError(f"{kind}: unknown parameters {sorted(unknown)}")
        vals.update(params or {})
        d = cls._FX_DESCS[kind]() if into is None else into
        d.width, d.height = int(W), int(H)
        if kind == "dof":
            d.blur_iterations, d.autofocus_radius = int(vals["iterations"]), int(vals["radius"])
            d.focus_x, d.focus_y = (W // 2, H // 2) if vals["focus"] is None else vals["focus"]
            d.range, d.max_blur = float(vals["range_"]), float(vals["max_blur"])
            return d
        if kind == "lens_flare":
            scales = [float(s) for s in vals.pop("ghost_scales")]
            if len(scales) > _abi.CANVAS_MAX_FLARE_GHOSTS:
                raise ValueError(f"lens_flare: at most {_abi.CANVAS_MAX_FLARE_GHOSTS} ghosts")
            d.n_ghosts = len(scales)
            for k in range(_abi.CANVAS_MAX_FLARE_GHOSTS):
                d.ghost_scales[k] = scales[k] if k < len(scales) else 0.0
        for name, v in vals.items():
            if name in ("curr_view", "curr_proj", "prev_view", "prev_proj"):
                if v is None:
                    raise TypeError(f"motion_blur: {name} is required")
                getattr(d, name)[:] = [float(f) for f in np.asarray(v, np.float32).reshape(16)]
            elif name == "fog_color":
                d.fog_color[:] = [int(c) for c in v]
            elif isinstance(getattr(d, name), int):
                setattr(d, name, int(v))
            else:
                setattr(d, name, float(v))
        return d

    def _fx_call(self, fn, desc, inputs, like, dst, prequant, H, W):
        """One post-pass entry: inputs (arrays or tensors, all where `like` lives) -> dst [, prequant]."""
        dev = _is_device(like)
        if any(_is_device(a) != dev for a in inputs):
            raise ValueError("canvas pass: every buffer must live where the first does")
        if dev:
            self._on_torch_stream()
        if dst is None:
            if dev:
                import torch
                dst = torch.empty((H, W, 4), dtype=torch.uint8, device=like.device)
            else:
                dst = np.empty((H, W, 4), np.uint8)
        args = [_ptr(a) for a in inputs] + [_ptr(dst)]
        pq = None
        if prequant is not None:
            if prequant:
                if dev:
                    import torch
                    pq = torch.empty((H, W, 4), dtype=torch.float32, device=like.device)
                else:
                    pq = np.empty((H, W, 4), np.float32)
            args.append(None if pq is None else _ptr(pq))
        self._check(fn(self._h, ctypes.byref(desc), *args, self.CANVAS_DEVICE if dev else 0))
        return (dst, pq) if prequant else dst

    def canvas_velocity_blur(self, src, velocity, samples=12, strength=1.0, dst=None):
        """motion_blur_pass (hello_multi_pass.cpp:605-683): src uint8 [H, W, 4], velocity float32 [H, W, 2] -> dst.
        Host arrays (synchronous) or torch CUDA tensors (asynchronous on the context stream), as every canvas pass."""
        H, W = src.shape[:2]
        d = self.fx_desc("velocity_blur", W, H, dict(samples=samples, strength=strength))
        return self._fx_call(self._lib.shs_canvas_velocity_blur, d, [_host_c(src, np.uint8), _host_c(velocity, np.float32)],
                             src, dst, None, H, W)

    def canvas_fog(self, src, depth, fog_color=(28, 30, 38, 255), fog_start=20.0, fog_end=80.0, fog_power=1.25, dst=None,
                   prequant=False):
        """fog_pass (hello_multi_pass.cpp:764-819); dst may be src.  prequant: also float32 [H, W, 4], the three sums
        before the byte conversion and 1 ((0, 0, 0, -1): an empty pixel, copied)."""
        H, W = src.shape[:2]
        d = self.fx_desc("fog", W, H, dict(fog_color=fog_color, fog_start=fog_start, fog_end=fog_end, fog_power=fog_power))
        return self._fx_call(self._lib.shs_canvas_fog, d, [_host_c(src, np.uint8), _host_c(depth, np.float32)], src, dst,
                             bool(prequant), H, W)

    def canvas_outline(self, src, depth, radius=1, threshold=0.75, strength=0.15, dst=None):
        """outline_pass (hello_multi_pass.cpp:689-758)."""
        H, W = src.shape[:2]
        d = self.fx_desc("outline", W, H, dict(radius=radius, threshold=threshold, strength=strength))
        return self._fx_call(self._lib.shs_canvas_outline, d, [_host_c(src, np.uint8), _host_c(depth, np.float32)], src, dst,
                             None, H, W)

    def canvas_fxaa(self, src, reduce_min=1.0 / 128.0, reduce_mul=1.0 / 8.0, span_max=8.0, dst=None):
        """fxaa_pass (hello_multi_pass.cpp:1000-1114)."""
        H, W = src.shape[:2]
        d = self.fx_desc("fxaa", W, H, dict(reduce_min=reduce_min, reduce_mul=reduce_mul, span_max=span_max))
        return self._fx_call(self._lib.shs_canvas_fxaa, d, [_host_c(src, np.uint8)], src, dst, None, H, W)

    def canvas_spec_bright(self, spec01, threshold=0.139, intensity=13.25, dst=None):
        """build_spec_bright_pass (hello_glowing_star.cpp:700-752): spec01 float32 [H, W] -> uint8 [H, W, 4]."""
        H, W = spec01.shape[:2]
        d = self.fx_desc("spec_bright", W, H, dict(threshold=threshold, intensity=intensity))
        return self._fx_call(self._lib.shs_canvas_spec_bright, d, [_host_c(spec01, np.float32)], spec01, dst, None, H, W)

    def canvas_additive(self, base, add, strength=1.0, out=None):
        """additive_composite_pass (hello_glowing_star.cpp:754-795); out may be base."""
        H, W = base.shape[:2]
        dev = _is_device(base)
        if _is_device(add) != dev:
            raise ValueError("canvas_additive: add must live where base does")
        if dev:
            self._on_torch_stream()
        if out is None:
            out = _empty_like(base)
        base, add = _host_c(base, np.uint8), _host_c(add, np.uint8)
        self._check(self._lib.shs_canvas_additive(self._h, W, H, _ptr(base), _ptr(add), float(strength), _ptr(out),
                                                  self.CANVAS_DEVICE if dev else 0))
        return out

    def canvas_lens_flare(self, src, intensity=0.55, halo_intensity=0.35, chroma_shift_px=0.8, ghost_scales=(0.55, 0.85, 1.25),
                          dst=None, prequant=False):
        """pseudo_lens_flare_pass (hello_glowing_star.cpp:802-906) over the bloom canvas.  prequant: also float32
        [H, W, 4], rr / gg / bb before the clamp and 1."""
        H, W = src.shape[:2]
        d = self.fx_desc("lens_flare", W, H, dict(intensity=intensity, halo_intensity=halo_intensity,
                                                  chroma_shift_px=chroma_shift_px, ghost_scales=ghost_scales))
        return self._fx_call(self._lib.shs_canvas_lens_flare, d, [_host_c(src, np.uint8)], src, dst, bool(prequant), H, W)

    def canvas_object_blur(self, src, depth, velocity, dst=None, **params):
        """post_process_motion_blur (hello_per_object_motion_blur.cpp:461-552): src uint8 [H, W, 4], depth float32 [H, W]
        (FLT_MAX = empty), velocity float32 [H, W, 2] (+Y up) -> dst.  params over FX_DEFAULTS["object_blur"]; depth_rows 1
        (the default): depth is in screen rows, what rt_render_plain leaves; 0: in canvas rows like src."""
        H, W = src.shape[:2]
        d = self.fx_desc("object_blur", W, H, params)
        return self._fx_call(self._lib.shs_canvas_object_blur, d,
                             [_host_c(src, np.uint8), _host_c(depth, np.float32), _host_c(velocity, np.float32)], src, dst, None, H, W)

    def canvas_ping_pong_blur(self, color, iterations=3):
        """hello_ping_pong.cpp:611-618: iterations x (horizontal, vertical) canvas_gaussian_blur on color in place, over a
        scratch canvas the context owns -> color."""
        H, W = color.shape[:2]
        dev = _is_device(color)
        if dev:
            self._on_torch_stream()
        self._check(self._lib.shs_canvas_ping_pong_blur(self._h, W, H, int(iterations), _ptr(color), self.CANVAS_DEVICE if dev else 0))
        return color

    def multi_pass_frame_desc(self, W, H, blur_mode=0, enable_dof=True, enable_fxaa=True, **passes):
        d = _abi.CanvasMultiPassFrameDescC()
        d.width, d.height, d.blur_mode = int(W), int(H), int(blur_mode)
        d.enable_dof, d.enable_fxaa = int(bool(enable_dof)), int(bool(enable_fxaa))
        unknown = set(passes) - {"velocity_blur", "motion_blur", "dof", "fog", "outline", "fxaa"}
        if unknown:
            raise TypeError(f"canvas_multi_pass_frame: unknown passes {sorted(unknown)}")
        for kind in ("velocity_blur", "dof", "fog", "outline", "fxaa"):
            self.fx_desc(kind, W, H, passes.get(kind), into=getattr(d, kind))
        if blur_mode != _abi.CANVAS_BLUR_VELOCITY_FIRST:
            self.fx_desc("motion_blur", W, H, passes.get("motion_blur"), into=d.motion_blur)
        return d

    def canvas_multi_pass_frame(self, color, depth, velocity, blur_mode=0, enable_dof=True, enable_fxaa=True, dst=None,
                                **passes):
        """A whole post chain in one call (include/shs_gpu.h): blur_mode 0 hello_multi_pass.cpp:1379-1426 (velocity
        blur, DoF, fog, outline, FXAA), 1 the same with canvas_motion_blur first, 2
        hello_camera_and_perobject_motion_blur.cpp's order (DoF, fog, outline, canvas_motion_blur, FXAA).  passes:
        velocity_blur=, motion_blur=, dof=, fog=, outline=, fxaa= dicts over FX_DEFAULTS (motion_blur needs the four
        matrices).  color is only read; dst may be color."""
        H, W = color.shape[:2]
        d = self.multi_pass_frame_desc(W, H, blur_mode, enable_dof, enable_fxaa, **passes)
        return self._fx_call(self._lib.shs_canvas_multi_pass_frame, d,
                             [_host_c(color, np.uint8), _host_c(depth, np.float32), _host_c(velocity, np.float32)], color, dst,
                             None, H, W)

    # hello_glowing_star.cpp:62-73: the star's blur and DoF constants
    GLOW_DEFAULTS = {"velocity_blur": dict(samples=8, strength=1.5), "dof": dict(iterations=3, range_=22.0, max_blur=0.80)}

    def glow_frame_desc(self, W, H, enable_dof=True, enable_bloom=True, enable_flare=True, bloom_iterations=10, **passes):
        d = _abi.CanvasGlowFrameDescC()
        d.width, d.height, d.bloom_iterations = int(W), int(H), int(bloom_iterations)
        d.enable_dof, d.enable_bloom, d.enable_flare = int(bool(enable_dof)), int(bool(enable_bloom)), int(bool(enable_flare))
        unknown = set(passes) - {"velocity_blur", "dof", "spec_bright", "lens_flare"}
        if unknown:
            raise TypeError(f"canvas_glow_frame: unknown passes {sorted(unknown)}")
        for kind in ("velocity_blur", "dof", "spec_bright", "lens_flare"):
            self.fx_desc(kind, W, H, dict(self.GLOW_DEFAULTS.get(kind, {}), **(passes.get(kind) or {})), into=getattr(d, kind))
        return d

    def canvas_glow_frame(self, color, depth, velocity, spec01, enable_dof=True, enable_bloom=True, enable_flare=True,
                          bloom_iterations=10, dst=None, **passes):
        """hello_glowing_star.cpp:1233-1310 in one call: velocity blur, DoF, bright pass over spec01 (float32 [H, W]),
        bloom_iterations x (horizontal, vertical) Gaussian, flare, two additive composites.  passes: velocity_blur=,
        dof=, spec_bright=, lens_flare= dicts over GLOW_DEFAULTS and FX_DEFAULTS."""
        H, W = color.shape[:2]
        d = self.glow_frame_desc(W, H, enable_dof, enable_bloom, enable_flare, bloom_iterations, **passes)
        return self._fx_call(self._lib.shs_canvas_glow_frame, d,
                             [_host_c(color, np.uint8), _host_c(depth, np.float32), _host_c(velocity, np.float32),
                              _host_c(spec01, np.float32)], color, dst, None, H, W)

    # -- Canvas render-target raster (hello_shadow_mapping.cpp PASS0 / PASS1) ---------------------
    def _rt_draw_array(self, draws):
        arr = (_abi.RtDrawC * max(len(draws), 1))()
        for i, d in enumerate(draws):
            arr[i].mesh_id = d.mesh if isinstance(d.mesh, int) else self.upload_mesh(d.mesh)
            tex = d.albedo_tex
            arr[i].albedo_tex = 0 if tex is None else (int(tex) if isinstance(tex, (int, np.integer)) else self.upload_texture(tex))
            for name in ("model", "mvp", "prev_mvp"):
                m = getattr(d, name)
                if m is not None:
                    getattr(arr[i], name)[:] = [float(v) for v in np.asarray(m, dtype=np.float32).reshape(16)]
            for k in range(4):
                arr[i].base_color[k] = int(d.base_color[k])
        return arr

    def rt_render_shadow(self, size, light_vp, casters, ref_tile=(80, 80)):
        """shs_rt_render_shadow: PASS0 over a size = (w, h) map (an int: square), asynchronous."""
        w, h = (size, size) if isinstance(size, int) else size
        lvp = np.ascontiguousarray(light_vp, dtype=np.float32).reshape(16)
        arr = self._rt_draw_array(casters)
        self._check(self._lib.shs_rt_render_shadow(self._h, w, h, ref_tile[0], ref_tile[1], _fptr(lvp), arr, len(casters)))
        self._rt_shadow_size = (w, h)

    def rt_render(self, frame, draws):
        """shs_rt_render: PASS1 (colour, view-z depth, velocity; the shadow lookup), asynchronous."""
        arr = self._rt_draw_array(draws)
        self._check(self._lib.shs_rt_render(self._h, ctypes.byref(self._rt_frame_c(frame)), arr, len(draws)))
        self._rt_size = (frame.width, frame.height)

    def _rt_frame_c(self, frame):
        f = _abi.RtFrameC()
        f.width, f.height = frame.width, frame.height
        f.ref_tile_w, f.ref_tile_h = frame.ref_tile
        for k in range(4):
            f.clear_color[k] = int(frame.clear_color[k])
        f.view[:] = [float(v) for v in np.asarray(frame.view, dtype=np.float32).reshape(16)]
        f.light_vp[:] = [float(v) for v in np.asarray(frame.light_vp, dtype=np.float32).reshape(16)]
        f.light_dir_world[:] = [float(v) for v in frame.light_dir_world]
        f.camera_pos[:] = [float(v) for v in frame.camera_pos]
        f.bias_base, f.bias_slope, f.max_velocity_px = frame.bias_base, frame.bias_slope, frame.max_velocity_px
        f.flags = (_abi.RT_USE_SHADOW if frame.use_shadow else 0) | (_abi.RT_PCF if frame.pcf else 0) | \
                  (_abi.RT_PREQUANT if frame.prequant else 0)
        f.shading = int(frame.shading)
        return f

    def rt_render_pbr(self, frame, draws, pbr_draws):
        """shs_rt_render_pbr: PASS1 of hello_pbr.cpp (frame.shading 2; pbr_draws: one RtPbrDraw per draw), asynchronous."""
        self._rt_render_pbr(self._lib.shs_rt_render_pbr, "rt_render_pbr", frame, draws, pbr_draws)

    def rt_render_pbr_soft(self, frame, draws, pbr_draws):
        """shs_rt_render_pbr_soft: PASS1 of hello_pbr_light_shafts.cpp (frame.shading 3: the PBR shader under the PCSS
        factor of rt_set_pcss, without the minimum ambient; pbr_draws: one RtPbrDraw per draw), asynchronous."""
        self._rt_render_pbr(self._lib.shs_rt_render_pbr_soft, "rt_render_pbr_soft", frame, draws, pbr_draws)

    def _rt_render_pbr(self, entry, name, frame, draws, pbr_draws):
        if len(pbr_draws) != len(draws):
            raise ShsError(-1, name + ": one RtPbrDraw per draw")
        arr = self._rt_draw_array(draws)
        mat = (_abi.RtPbrDrawC * max(len(draws), 1))()
        for i, m in enumerate(pbr_draws):
            n3 = np.eye(3, dtype=np.float32).reshape(9) if m.normal_mat is None else np.asarray(m.normal_mat, np.float32).reshape(9)
            mat[i].normal_mat[:] = [float(v) for v in n3]
            for name in ("metallic", "roughness", "ao", "ibl_diffuse_intensity", "ibl_specular_intensity", "ibl_reflection_strength"):
                setattr(mat[i], name, float(getattr(m, name)))
        self._check(entry(self._h, ctypes.byref(self._rt_frame_c(frame)), arr, mat, len(draws)))
        self._rt_size = (frame.width, frame.height)

    def rt_render_skybox_ibl(self, frame, draws, ibl_draws):
        """shs_rt_render_skybox_ibl: PASS1 of hello_ibl_skybox.cpp (frame.shading 4: Blinn-Phong under the shadow lookup,
        tinted by and reflecting the sky of rt_set_sky; ibl_draws: one RtSkyboxIblDraw per draw, or None to hand the
        library a null table), asynchronous."""
        arr = self._rt_draw_array(draws)
        knobs = None
        if ibl_draws is not None:
            if len(ibl_draws) != len(draws):
                raise ShsError(-1, "rt_render_skybox_ibl: one RtSkyboxIblDraw per draw")
            knobs = (_abi.RtSkyboxIblDrawC * max(len(draws), 1))()
            for i, k in enumerate(ibl_draws):
                knobs[i] = _abi.RtSkyboxIblDrawC(float(k.ibl_ambient), float(k.ibl_refl), float(k.ibl_f0), float(k.ibl_refl_mix))
        self._check(self._lib.shs_rt_render_skybox_ibl(self._h, ctypes.byref(self._rt_frame_c(frame)), arr, knobs, len(draws)))
        self._rt_size = (frame.width, frame.height)

    def rt_render_ibl_phong(self, frame, draws, ibl_draws):
        """shs_rt_render_ibl_phong: PASS1 of hello_ibl_skybox_optimized.cpp / hello_ibl_skybox_xsimd.cpp (frame.shading 11:
        Blinn-Phong with a per-draw shininess under the shadow lookup, plus the irradiance and prefiltered-specular terms
        of the IBL of rt_set_ibl; ibl_draws: one RtIblPhongDraw per draw, or None to hand the library a null table),
        asynchronous."""
        arr = self._rt_draw_array(draws)
        knobs = None
        if ibl_draws is not None:
            if len(ibl_draws) != len(draws):
                raise ShsError(-1, "rt_render_ibl_phong: one RtIblPhongDraw per draw")
            knobs = (_abi.RtIblPhongDrawC * max(len(draws), 1))()
            for i, k in enumerate(ibl_draws):
                knobs[i] = _abi.RtIblPhongDrawC(float(k.ibl_ambient), float(k.ibl_refl), float(k.ibl_f0), float(k.ibl_refl_mix),
                                                float(k.shininess))
        self._check(self._lib.shs_rt_render_ibl_phong(self._h, ctypes.byref(self._rt_frame_c(frame)), arr, knobs, len(draws)))
        self._rt_size = (frame.width, frame.height)

    def rt_render_shadow_edge(self, size, light_vp, casters, ref_tile=(160, 160), lanes=8):
        """shs_rt_render_shadow_edge: PASS0 of hello_ibl_skybox_xsimd.cpp (the edge-function raster; lanes: the reference
        build's xsimd::batch<float>::size) over a size = (w, h) map (an int: square), asynchronous."""
        w, h = (size, size) if isinstance(size, int) else size
        lvp = np.ascontiguousarray(light_vp, dtype=np.float32).reshape(16)
        arr = self._rt_draw_array(casters)
        self._check(self._lib.shs_rt_render_shadow_edge(self._h, w, h, ref_tile[0], ref_tile[1], _fptr(lvp), arr, len(casters), int(lanes)))
        self._rt_shadow_size = (w, h)

    def rt_render_water(self, frame, draws, water_draws, water):
        """shs_rt_render_water: PASS1A / PASS1B of hello_water.cpp (frame.shading 5; water_draws: one RtWaterDraw per draw, or
        None to hand the library a null table; water: an RtWater), asynchronous."""
        arr = self._rt_draw_array(draws)
        flags = None
        if water_draws is not None:
            if len(water_draws) != len(draws):
                raise ShsError(-1, "rt_render_water: one RtWaterDraw per draw")
            flags = (_abi.RtWaterDrawC * max(len(draws), 1))()
            for i, k in enumerate(water_draws):
                flags[i].flags = int(k) if isinstance(k, (int, np.integer)) else (_abi.RT_WATER_SURFACE if k.surface else 0)
        wc = None
        if water is not None:
            wc = _abi.RtWaterC()
            vp = np.eye(4, dtype=np.float32) if water.reflection_vp is None else np.asarray(water.reflection_vp, np.float32)
            wc.reflection_vp[:] = [float(v) for v in vp.reshape(16)]
            wc.time_sec = float(water.time_sec)
            r = water.reflection
            wc.flags = int(r) if isinstance(r, (int, np.integer)) and not isinstance(r, bool) else (_abi.RT_WATER_REFLECTION if r else 0)
            wc = ctypes.byref(wc)
        self._check(self._lib.shs_rt_render_water(self._h, ctypes.byref(self._rt_frame_c(frame)), arr, flags, wc, len(draws)))
        self._rt_size = (frame.width, frame.height)

    def rt_render_motion(self, frame, draws):
        """shs_rt_render_motion: the unclipped camera pass of hello_multi_pass.cpp / hello_camera_and_perobject_motion_blur.cpp
        (frame.shading 6) and hello_glowing_star.cpp (frame.shading 7, which also fills the spec plane), asynchronous."""
        arr = self._rt_draw_array(draws)
        self._check(self._lib.shs_rt_render_motion(self._h, ctypes.byref(self._rt_frame_c(frame)), arr, len(draws)))
        self._rt_size = (frame.width, frame.height)

    def rt_render_plain(self, frame, draws):
        """shs_rt_render_plain: the unclipped camera pass of hello_per_object_motion_blur.cpp (frame.shading 8, velocity per
        pixel), hello_depth_of_field.cpp (9) and hello_ping_pong.cpp (10, NDC-z depth), asynchronous.  The depth plane it
        leaves is in SCREEN rows (row 0 is the top of the screen); every other plane is in canvas rows."""
        arr = self._rt_draw_array(draws)
        self._check(self._lib.shs_rt_render_plain(self._h, ctypes.byref(self._rt_frame_c(frame)), arr, len(draws)))
        self._rt_size = (frame.width, frame.height)

    def rt_resolve_spec(self):
        """-> spec01 float32 [H, W] of the last shading-7 frame, canvas rows (0 where no fragment is shown)."""
        W, H = self._rt_dims()
        spec = np.empty((H, W), np.float32)
        self._check(self._lib.shs_rt_resolve_spec(self._h, _ptr(spec)))
        return spec

    def rt_device_spec(self):
        """Device pointer of the last shading-7 frame's spec plane (W*H float32)."""
        a = ctypes.c_void_p()
        self._check(self._lib.shs_rt_device_spec(self._h, ctypes.byref(a)))
        return a.value

    def rt_keep_reflection(self):
        """shs_rt_keep_reflection: the last camera pass's colour plane becomes the reflection canvas, asynchronous."""
        self._check(self._lib.shs_rt_keep_reflection(self._h))

    def rt_set_reflection(self, rgba=None):
        """shs_rt_set_reflection: the reflection canvas from a host image uint8 [h, w, 4] in canvas rows (None: none)."""
        if rgba is None:
            self._check(self._lib.shs_rt_set_reflection(self._h, None, 0, 0))
            return
        rgba = np.ascontiguousarray(rgba, np.uint8)
        if rgba.ndim != 3 or rgba.shape[2] != 4:
            raise ShsError(-1, f"rt_set_reflection: an image of shape {rgba.shape}")
        self._check(self._lib.shs_rt_set_reflection(self._h, _ptr(rgba), rgba.shape[1], rgba.shape[0]))

    def rt_water_samples(self, world_pos, time_sec):
        """shs_rt_water_samples: water_flow_normal_and_foam of n points -> (normal float32 [n, 3], foam float32 [n])."""
        pos = np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3)
        n = pos.shape[0]
        nrm, foam = np.empty((n, 3), np.float32), np.empty(n, np.float32)
        self._check(self._lib.shs_rt_water_samples(self._h, n, _ptr(pos), float(time_sec), _ptr(nrm), _ptr(foam)))
        return nrm, foam

    def rt_set_pbr(self, pbr=None):
        """shs_rt_set_pbr: the constants of shadings 2 and 3 (an RtPbr; None: the demo's)."""
        if pbr is None:
            self._check(self._lib.shs_rt_set_pbr(self._h, None))
            return
        c = _abi.RtPbrC(pbr.exposure, pbr.min_roughness, pbr.direct_intensity)
        self._check(self._lib.shs_rt_set_pbr(self._h, ctypes.byref(c)))

    def rt_set_ibl(self, irr=None, spec_mips=None):
        """shs_rt_set_ibl: irr float32 [6, n, n, 3] and spec_mips a list of [6, s_m, s_m, 3] with
        s_m = max(1, s_0 >> m); irr None: no IBL.  Synchronous."""
        if irr is None:
            self._check(self._lib.shs_rt_set_ibl(self._h, 0, None, 0, 0, None))
            return
        irr = np.ascontiguousarray(irr, np.float32)
        mips = [np.ascontiguousarray(m, np.float32) for m in spec_mips]
        base = mips[0].shape[1] if mips else 0
        for m, a in enumerate([irr] + mips):
            want = irr.shape[1] if m == 0 else max(1, base >> (m - 1))
            if a.ndim != 4 or a.shape != (6, want, want, 3):
                raise ShsError(-1, f"rt_set_ibl: level {m} has shape {a.shape}")
        spec = np.concatenate([m.reshape(-1) for m in mips]) if mips else np.zeros(0, np.float32)
        one = np.zeros(1, np.float32)       # (an empty level still goes down as a pointer: the library rejects the size)
        self._check(self._lib.shs_rt_set_ibl(self._h, irr.shape[1], _ptr(irr if irr.size else one), base, len(mips),
                                             _ptr(spec if spec.size else one)))

    def rt_ibl_samples(self, dirs, lod):
        """shs_rt_ibl_samples: (irradiance at dir, trilinear prefiltered specular at (dir, lod)) -> two float32 [n, 3]."""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = dirs.shape[0]
        lod = np.ascontiguousarray(lod, np.float32).reshape(n)
        a, b = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        self._check(self._lib.shs_rt_ibl_samples(self._h, n, _ptr(dirs), _ptr(lod), _ptr(a), _ptr(b)))
        return a, b

    def rt_set_sky(self, sky=None):
        """shs_rt_set_sky: the sky later camera passes draw behind the triangles (an RtSky; None: no sky, uncovered
        pixels keep clear_color)."""
        if sky is None:
            self._check(self._lib.shs_rt_set_sky(self._h, None))
            return
        c = _abi.RtSkyC()
        c.model, c.encode = int(sky.model), int(sky.encode)
        c.intensity, c.fov_degrees, c.exposure = float(sky.intensity), float(sky.fov_degrees), float(sky.exposure)
        for name in ("sun_dir", "cam_forward", "cam_right", "cam_up"):
            getattr(c, name)[:] = [float(v) for v in getattr(sky, name)]
        for k, tex in enumerate(tuple(sky.face_tex)[:6]):
            c.face_tex[k] = int(tex) if isinstance(tex, (int, np.integer)) else self.upload_texture(tex)
        self._check(self._lib.shs_rt_set_sky(self._h, ctypes.byref(c)))

    def rt_sky_samples(self, dirs):
        """shs_rt_sky_samples: the bound sky's linear radiance sky.sample(dir) -> float32 [n, 3], synchronous."""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.empty_like(dirs)
        self._check(self._lib.shs_rt_sky_samples(self._h, dirs.shape[0], _ptr(dirs), _ptr(out)))
        return out

    def rt_set_pcss(self, pcss=None):
        """shs_rt_set_pcss: the PCSS constants of shadings 1 and 3 (an RtPcss; None: the demo's)."""
        if pcss is None:
            self._check(self._lib.shs_rt_set_pcss(self._h, None))
            return
        c = _abi.RtPcssC(pcss.light_uv_radius, pcss.search_radius_texels, pcss.min_filter_texels, pcss.max_filter_texels,
                         pcss.epsilon, int(pcss.blocker_samples), int(pcss.pcf_samples))
        self._check(self._lib.shs_rt_set_pcss(self._h, ctypes.byref(c)))

    def rt_pcss_samples(self, shadow_map, uv, z, bias, pxpy):
        """shs_rt_pcss_samples: pcss_shadow_factor of n samples over a host map [h, w] -> float32 [n], synchronous."""
        sm = np.ascontiguousarray(shadow_map, np.float32)
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n = uv.shape[0]
        z = np.ascontiguousarray(z, np.float32).reshape(n)
        bias = np.ascontiguousarray(bias, np.float32).reshape(n)
        pxpy = np.ascontiguousarray(pxpy, np.int32).reshape(n, 2)
        out = np.empty(n, np.float32)
        self._check(self._lib.shs_rt_pcss_samples(self._h, _ptr(sm), sm.shape[1], sm.shape[0], n, _ptr(uv), _ptr(z), _ptr(bias),
                                                  _ptr(pxpy), _ptr(out)))
        return out

    def _rt_dims(self, shadow=False):
        size = self._rt_shadow_size if shadow else self._rt_size
        if size is None:
            raise ShsError(-1, "no render-target shadow map rendered" if shadow else "no render-target frame rendered")
        return size

    def rt_resolve(self):
        """-> (color uint8 [H, W, 4], depth float32 [H, W], velocity float32 [H, W, 2]), canvas rows."""
        W, H = self._rt_dims()
        color = np.empty((H, W, 4), np.uint8)
        depth = np.empty((H, W), np.float32)
        vel = np.empty((H, W, 2), np.float32)
        self._check(self._lib.shs_rt_resolve(self._h, _ptr(color), _ptr(depth), _ptr(vel)))
        return color, depth, vel

    def rt_resolve_shadow(self):
        w, h = self._rt_dims(shadow=True)
        sm = np.empty((h, w), np.float32)
        self._check(self._lib.shs_rt_resolve_shadow(self._h, _ptr(sm)))
        return sm

    def rt_resolve_prequant(self):
        W, H = self._rt_dims()
        pq = np.empty((H, W, 4), np.float32)
        self._check(self._lib.shs_rt_resolve_prequant(self._h, _ptr(pq)))
        return pq

    def rt_resolve_ids(self):
        W, H = self._rt_dims()
        ids = np.empty((H, W), np.int32)
        self._check(self._lib.shs_rt_resolve_ids(self._h, _ptr(ids)))
        return ids

    def rt_stats(self) -> dict:
        st = _abi.RtStatsC()
        self._check(self._lib.shs_rt_get_stats(self._h, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def rt_device_targets(self):
        """Device pointers of the last camera pass: (colour W*H*4 bytes, depth W*H, velocity float2 W*H)."""
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.shs_rt_device_targets(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def rt_device_shadow_map(self):
        """-> (device address of the last rt_render_shadow's map, (w, h)): w * h float32, y down."""
        a, w, h = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._lib.shs_rt_device_shadow_map(self._h, ctypes.byref(a), ctypes.byref(w), ctypes.byref(h)))
        return a.value, (w.value, h.value)

    def lib_device_targets(self):
        """Device pointers of the library targets: (hdr float4 W*H, depth W*H, motion float2 W*H)."""
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.shs_lib_device_targets(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def ldr_device_targets(self):
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.shs_ldr_device_targets(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    @staticmethod
    def tonemap_thresholds(gamma: float):
        """Host-side byte thresholds in x = c / (1 + c) (thr[0] = 0; +inf = byte never reached)."""
        thr = np.zeros(256, np.float32)
        rc = lib().shs_tonemap_thresholds(float(gamma), thr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        if rc != 0:
            raise ShsError(rc, "shs_tonemap_thresholds")
        return thr

    @staticmethod
    def shard_balance(blocks, width, height, count, root_share=1.0):
        """Host-side region balance (shs_shard_balance_rects): blocks uint32 [n, 4] as k_lib_setup writes them
        -> [(bx0, by0, bx1, by1)] per rank."""
        b = np.ascontiguousarray(np.asarray(blocks, np.uint32).reshape(-1, 4))
        out = np.zeros(4 * count, np.int32)
        rc = lib().shs_shard_balance_rects(b.ctypes.data if b.size else None, b.shape[0], int(width), int(height), int(count),
                                           int(round(root_share * 1000)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        if rc != 0:
            raise ShsError(rc, "shs_shard_balance_rects")
        return [tuple(int(v) for v in out[4 * r:4 * r + 4]) for r in range(count)]

    @staticmethod
    def shadow_footprint(light_vp, sm_size, camera_vp, width, height, px_rect, world_min, world_max, reach):
        """Host-side footprint (shs_shadow_footprint): the texel rectangle (x0, y0, x1, y1), inclusive, of an
        sm_size = (w, h) shadow map that PCF of `reach` texels reads from the points of the world box whose
        camera projection lands on px_rect (x0, y0, x1, y1; rows y up) of a width x height frame."""
        sw, sh = (sm_size, sm_size) if isinstance(sm_size, int) else sm_size
        f16 = lambda m: np.ascontiguousarray(np.asarray(m, np.float32).reshape(16))
        f3 = lambda v: np.ascontiguousarray(np.asarray(v, np.float32).reshape(3))
        lv, cv, b0, b1 = f16(light_vp), f16(camera_vp), f3(world_min), f3(world_max)
        px = np.ascontiguousarray(np.asarray(px_rect, np.int32).reshape(4))
        out = np.zeros(4, np.int32)
        rc = lib().shs_shadow_footprint(lv.ctypes.data, int(sw), int(sh), cv.ctypes.data, int(width), int(height),
                                        px.ctypes.data, b0.ctypes.data, b1.ctypes.data, int(reach), out.ctypes.data)
        if rc != 0:
            raise ShsError(rc, "shs_shadow_footprint")
        return tuple(int(v) for v in out)

    @staticmethod
    def shadow_footprint_rows(light_vp, sm_size, camera_vp, width, height, px_rect, world_min, world_max, reach,
                              row_h=32):
        """shs_shadow_footprint_rows: per row of row_h texels the read texel columns -> (x0[], x1[]) int32
        arrays (x1 < x0: none), from the footprint polytope's convex light-space image."""
        sw, sh = (sm_size, sm_size) if isinstance(sm_size, int) else sm_size
        f16 = lambda m: np.ascontiguousarray(np.asarray(m, np.float32).reshape(16))
        f3 = lambda v: np.ascontiguousarray(np.asarray(v, np.float32).reshape(3))
        lv, cv, b0, b1 = f16(light_vp), f16(camera_vp), f3(world_min), f3(world_max)
        px = np.ascontiguousarray(np.asarray(px_rect, np.int32).reshape(4))
        n_rows = (int(sh) + row_h - 1) // row_h
        x0, x1 = np.zeros(n_rows, np.int32), np.zeros(n_rows, np.int32)
        rc = lib().shs_shadow_footprint_rows(lv.ctypes.data, int(sw), int(sh), cv.ctypes.data, int(width), int(height),
                                             px.ctypes.data, b0.ctypes.data, b1.ctypes.data, int(reach), int(row_h),
                                             n_rows, x0.ctypes.data, x1.ctypes.data)
        if rc != 0:
            raise ShsError(rc, "shs_shadow_footprint_rows")
        return x0, x1

    LIB_TIMELINE_FIELDS = ("start", "end", "gather", "pairs", "shade", "clear", "n_busy", "n_clear", "chunks",
                           "n_pairs", "n_cand", "max_tile", "stage", "seg", "tiles", "last",
                           "mt_rt", "mt_items", "mt_rounds", "mt_passes", "mt_staged", "mt_pairs", "mt_gather",
                           "mt_breaks")

    def lib_debug_timeline(self):
        """Last camera pass's k_lib_raster workgroup timeline: uint64 [grid, 24] (LIB_TIMELINE_FIELDS;
        times in 10-ns ticks; mt_*: the workgroup's longest busy tile)."""
        n = ctypes.c_int64()
        self._check(self._lib.shs_lib_debug_timeline(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        self._check(self._lib.shs_lib_debug_timeline(self._h, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        return out.reshape(-1, len(self.LIB_TIMELINE_FIELDS))

    def lib_debug_setup_timeline(self):
        """Last camera pass's k_lib_setup workgroup timeline: uint64 [blocks, 8] (start, triangles done,
        deferred marks done, end in 10-ns ticks; large primitives; deferred union w*h; tile-sharded cull
        front end done (0 without it); kept triangles)."""
        n = ctypes.c_int64()
        self._check(self._lib.shs_lib_debug_setup_timeline(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        self._check(self._lib.shs_lib_debug_setup_timeline(self._h, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                           ctypes.byref(n)))
        return out.reshape(-1, 8)

    def debug_timeline(self):
        """Last frame's workgroup timeline: (header dict, setup [n,2], raster [n,2]) in 10-ns ticks."""
        n = ctypes.c_int64()
        self._check(self._lib.shs_debug_timeline(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        self._check(self._lib.shs_debug_timeline(self._h, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        hs, hr, stride = int(out[0]), int(out[1]), int(out[5])
        head = {"setup_grid": hs, "raster_grid": hr, "setup_blocks": int(out[2]), "ghost_blocks": int(out[3]),
                "clear_blocks": int(out[4])}
        slots = out[8:].reshape(-1, stride)
        return head, slots[:hs], slots[hs:hs + hr]

    def set_bin_capacity(self, cap: int):
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_BIN_CAPACITY, int(cap)))

    def set_lib_part(self, part: int):
        """Camera-pass raster work split (SHS_OPT_LIB_PART): -1 auto (512 when sharded), 0 off (default), else the part size."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_LIB_PART, int(part)))

    def set_shard_cull(self, on: bool):
        """SHS_OPT_SHARD_CULL: tile-sharded camera passes set up only the rank's triangles (default off)."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_SHARD_CULL, 1 if on else 0))

    def set_shard_layout(self, regions: bool):
        """SHS_OPT_SHARD_LAYOUT: tile-sharded library frames own interleaved 32x32 tiles (default) or one
        cost-balanced rectangle per rank (regions=True)."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_SHARD_LAYOUT,
                                             _abi.SHARD_REGIONS if regions else _abi.SHARD_INTERLEAVED))

    def set_shard_root_share(self, share: float):
        """SHS_OPT_SHARD_ROOT_SHARE: rank 0's share of a region layout relative to the others (0..1)."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_SHARD_ROOT_SHARE, int(round(share * 1000))))

    def set_legacy_pipeline(self, on: bool):
        """SHS_OPT_LEGACY_PIPELINE: a multi-draw scan-mode batch's raster runs in the next batch's launch
        (or at the next call that reads frames); results identical, frames final only after such a call."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_LEGACY_PIPELINE, 1 if on else 0))

    def set_stale_clear(self, on: bool):
        """SHS_OPT_LEGACY_STALE_CLEAR: legacy batches clear only the tiles an earlier batch left non-clear
        (default on); off: every batch clears every idle tile.  Images identical either way."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_LEGACY_STALE_CLEAR, 1 if on else 0))

    def set_tile_groups(self, on: bool):
        """SHS_OPT_LEGACY_TILE_GROUPS: scan-mode legacy batches raster their busy tiles in 2x2 groups that
        share one box scan and staging (default on); off: a work item per busy tile.  Images identical."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_LEGACY_TILE_GROUPS, 1 if on else 0))

    def set_group_spans(self, on: bool):
        """SHS_OPT_LEGACY_GROUP_SPANS: a tile group's pair pass walks conservative row spans of the
        candidates' clipped boxes (default on); off: the whole boxes.  Images identical."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_LEGACY_GROUP_SPANS, 1 if on else 0))

    def cleared_tiles(self) -> int:
        """shs_legacy_cleared_tiles: the 32x8 raster tiles the last legacy batch's clear strips cleared."""
        n = ctypes.c_uint64(0)
        self._check(self._lib.shs_legacy_cleared_tiles(self._h, ctypes.byref(n)))
        return int(n.value)

    def set_shadow_footprint(self, on: bool):
        """SHS_OPT_SHADOW_FOOTPRINT: shadow passes are recorded and rendered by the next camera pass over
        only the shadow-map tiles its pixels' PCF can read (default off: the whole map when called)."""
        self._check(self._lib.shs_set_option(self._h, _abi.OPT_SHADOW_FOOTPRINT, 1 if on else 0))

    def shadow_region(self):
        """The last enqueued shadow pass's bin tiles (bx0, by0, bx1, by1), inclusive; bx1 < bx0: none."""
        arr = (ctypes.c_int32 * 4)()
        self._check(self._lib.shs_get_shadow_region(self._h, arr))
        return tuple(arr)

    def shard_regions(self, count):
        """The last region-sharded camera pass's layout: [(bx0, by0, bx1, by1)] per rank (bin tiles, inclusive)."""
        arr = (ctypes.c_int32 * (4 * count))()
        self._check(self._lib.shs_get_shard_regions(self._h, count, arr))
        return [tuple(arr[4 * r:4 * r + 4]) for r in range(count)]

    def set_overflow_capacities(self, spill: int = 0, frags: int = 0):
        """Tests: shrink the legacy bin-spill / ghost-fragment lists (0 = leave) to force overflows."""
        if spill:
            self._check(self._lib.shs_set_option(self._h, _abi.OPT_SPILL_CAPACITY, int(spill)))
        if frags:
            self._check(self._lib.shs_set_option(self._h, _abi.OPT_FRAG_CAPACITY, int(frags)))

    def set_stream(self, hip_stream):
        self._check(self._lib.shs_set_stream(self._h, ctypes.c_void_p(hip_stream)))

    # -- library path (rasterize_mesh / PassShadowMap / PassPBRForward) ---------------------------
    def share_lib_mesh(self, src, mesh) -> int:
        """A handle to src's device copy of library mesh `mesh` (uploaded there if it is not yet), so
        that later draws of `mesh` on this context read src's buffers (shs_mesh_share: frames in flight
        on several contexts keep one copy).  src must outlive this context's use of it."""
        key = ("lib", id(mesh))
        if key in self._meshes:
            return self._meshes[key][0]
        sid = src.upload_lib_mesh(mesh)
        mid = ctypes.c_int32()
        self._check(self._lib.shs_mesh_share(self._h, src._h, sid, ctypes.byref(mid)))
        self._meshes[key] = (mid.value, mesh)
        return mid.value

    def upload_lib_mesh(self, mesh) -> int:
        key = ("lib", id(mesh))
        if key in self._meshes:
            return self._meshes[key][0]
        pos = np.ascontiguousarray(mesh.positions, dtype=np.float32).reshape(-1, 3)
        nrm = None if mesh.normals is None else np.ascontiguousarray(mesh.normals, dtype=np.float32).reshape(-1, 3)
        uv = None if mesh.uvs is None else np.ascontiguousarray(mesh.uvs, dtype=np.float32).reshape(-1, 2)
        idx = None if mesh.indices is None else np.ascontiguousarray(mesh.indices, dtype=np.uint32).reshape(-1)
        mid = ctypes.c_int32()
        self._check(self._lib.shs_mesh_upload(
            self._h, _fptr(pos), pos.shape[0],
            _fptr(nrm) if nrm is not None else None, 0 if nrm is None else nrm.shape[0],
            _fptr(uv) if uv is not None else None, 0 if uv is None else uv.shape[0],
            idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if idx is not None else None,
            0 if idx is None else idx.size, ctypes.byref(mid)))
        self._meshes[key] = (mid.value, mesh)
        return mid.value

    def render_shadow_map(self, size, sun_dir, casters):
        """PassShadowMap::execute -> the light camera's viewproj (float32[16])."""
        from ._abi import ShadowCasterC
        w, h = (size, size) if isinstance(size, int) else size
        arr = (ShadowCasterC * max(len(casters), 1))()
        for i, c in enumerate(casters):
            arr[i].mesh_id = c.mesh if isinstance(c.mesh, int) else self.upload_lib_mesh(c.mesh)
            for k in range(16):
                arr[i].model[k] = float(c.model[k])
        sd = np.ascontiguousarray(sun_dir, dtype=np.float32).reshape(3)
        vp = np.zeros(16, np.float32)
        self._check(self._lib.shs_render_shadow_map(self._h, w, h, _fptr(sd), arr, len(casters), _fptr(vp)))
        self._shadow_size = (w, h)
        return vp

    def resolve_shadow_map(self):
        w, h = self._shadow_size
        out = np.empty((h, w), np.float32)
        self._check(self._lib.shs_resolve_shadow_map(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def upload_texture(self, tex) -> int:
        """shs_texture_upload of a lib_path.Texture2D (cached per object) -> texture id (>= 1)."""
        key = ("tex", id(tex))
        if key in self._meshes:
            return self._meshes[key][0]
        rgba = np.ascontiguousarray(tex.rgba, dtype=np.uint8)
        assert rgba.ndim == 3 and rgba.shape[2] == 4
        tid = ctypes.c_int32()
        self._check(self._lib.shs_texture_upload(self._h, rgba.ctypes.data_as(ctypes.c_void_p), rgba.shape[1],
                                                 rgba.shape[0], ctypes.byref(tid)))
        self._meshes[key] = (tid.value, tex)
        return tid.value

    def prepare_lib(self, frame, draws):
        from ._abi import LibDrawC
        from .lib_path import fill_draw_struct
        arr = (LibDrawC * max(len(draws), 1))()
        for i, d in enumerate(draws):
            tex = getattr(d, "base_color_tex", None)
            fill_draw_struct(arr[i], d, d.mesh if isinstance(d.mesh, int) else self.upload_lib_mesh(d.mesh),
                             0 if tex is None else self.upload_texture(tex))
        return frame, frame.desc(), arr, len(draws)

    def render_pbr_forward_prepared(self, prepared):
        frame, desc, arr, n = prepared
        self._check(self._lib.shs_render_pbr_forward(self._h, ctypes.byref(desc), arr, n))
        self._lib_frame = frame

    def render_pbr_forward(self, frame, draws):
        """PassPBRForward::execute: clears + one rasterize_mesh per draw (asynchronous)."""
        self.render_pbr_forward_prepared(self.prepare_lib(frame, draws))

    def resolve_lib(self):
        """-> (hdr float32[H,W,4], depth float32[H,W] or None, motion float32[H,W,2] or None), rows y-up."""
        f = self._lib_frame
        hdr = np.empty((f.height, f.width, 4), np.float32)
        depth = np.empty((f.height, f.width), np.float32) if f.depth_motion else None
        motion = np.empty((f.height, f.width, 2), np.float32) if f.depth_motion else None
        vp = ctypes.c_void_p
        self._check(self._lib.shs_resolve_lib(self._h, hdr.ctypes.data_as(vp),
                                              depth.ctypes.data_as(vp) if depth is not None else None,
                                              motion.ctypes.data_as(vp) if motion is not None else None))
        return hdr, depth, motion

    def synchronize_lib(self):
        """Wait for the enqueued library passes (re-issues a pass whose capacity overflowed)."""
        from ._abi import LibStats
        if self._lib_frame is not None:
            self._check(self._lib.shs_get_lib_stats(self._h, ctypes.byref(LibStats())))
        elif self._shadow_size is not None:
            self.resolve_shadow_map()

    # -- tile shards (multi-GPU gather) ----------------------------------------------------------
    TARGET_LEGACY, TARGET_LIB, TARGET_PRESENT, TARGET_LIB_PRESENT = 0, 1, 2, 3

    def tiles_packed_words(self, target, count):
        """Packed words of the largest rank's tiles (a buffer size every rank's tiles fit)."""
        n = ctypes.c_int64()
        self._check(self._lib.shs_tiles_packed_words(self._h, target, count, ctypes.byref(n)))
        return n.value

    def tiles_rank_words(self, target, rank, count):
        """Packed words of rank's own tiles (region layouts differ per rank)."""
        n = ctypes.c_int64()
        self._check(self._lib.shs_tiles_rank_words(self._h, target, rank, count, ctypes.byref(n)))
        return n.value

    def tiles_pack(self, target, rank, count, dst_ptr):
        """Pack rank's owned tiles into the device buffer at dst_ptr (e.g. tensor.data_ptr())."""
        self._check(self._lib.shs_tiles_pack(self._h, target, rank, count, ctypes.c_void_p(dst_ptr)))

    def tiles_unpack(self, target, rank, count, src_ptr):
        self._check(self._lib.shs_tiles_unpack(self._h, target, rank, count, ctypes.c_void_p(src_ptr)))

    def tiles_unpack_ranks(self, target, count, src_ptrs):
        """shs_tiles_unpack_ranks: every rank's packed device buffer (src_ptrs[r]; 0 / None skips rank r)
        unpacked into this context's frame by one launch."""
        arr = (ctypes.c_void_p * count)(*[int(p) if p else None for p in src_ptrs])
        self._check(self._lib.shs_tiles_unpack_ranks(self._h, int(target), int(count), arr))

    def upload_lights(self, lights):
        """lights: numpy LIGHT_DTYPE array (CullingLightGPU records)."""
        from ._abi import CullingLightC
        arr = np.ascontiguousarray(lights)
        self._check(self._lib.shs_lights_upload(self._h, arr.ctypes.data_as(ctypes.POINTER(CullingLightC)), arr.shape[0]))
        self._n_lights = arr.shape[0]

    def upload_lights_typed(self, props):
        """props: numpy LIGHT_PROPS_DTYPE array (shs_light_props).  Packs the culling records
        (shs_light_pack_culling), uploads both (shs_lights_upload_typed: PROGRAM_FORWARD_PLUS_TYPED shades
        each light with the model of its type) and returns the culling records (LIGHT_DTYPE)."""
        from ._abi import CullingLightC, LightPropsC
        from .lib_path import LIGHT_PROPS_DTYPE, pack_culling
        arr = np.ascontiguousarray(props, dtype=LIGHT_PROPS_DTYPE)
        try:
            cull = pack_culling(arr)
        except ValueError as e:   # a type outside 1-4: what shs_lights_upload_typed itself answers
            raise ShsError(_abi.SHS_ERR_INVALID, str(e)) from None
        self._check(self._lib.shs_lights_upload_typed(self._h, cull.ctypes.data_as(ctypes.POINTER(CullingLightC)),
                                                      arr.ctypes.data_as(ctypes.POINTER(LightPropsC)), arr.shape[0]))
        self._n_lights = arr.shape[0]
        return cull

    def light_cull(self, cull):
        """fp_stress_light_cull.comp (+ depth reduce for mode 2) into the context's tile lists."""
        self._cull = cull
        self._check(self._lib.shs_light_cull(self._h, ctypes.byref(cull.desc())))

    def resolve_light_lists(self):
        """-> (counts uint32[n_lists], indices uint32[n_lists, max_per_tile], ranges float32[tiles, 2])."""
        c = self._cull
        counts = np.empty(c.n_lists, np.uint32)
        idx = np.empty((c.n_lists, c.max_per_tile), np.uint32)
        tx, ty = c.tiles
        ranges = np.empty((ty * tx, 2), np.float32)
        vp = ctypes.c_void_p
        self._check(self._lib.shs_resolve_light_lists(self._h, counts.ctypes.data_as(vp), idx.ctypes.data_as(vp),
                                                      ranges.ctypes.data_as(vp)))
        return counts, idx, ranges

    def light_bin_culling(self, lb, aabbs):
        """build_light_bin_culling on the GPU: lb = lib_path.LightBin, aabbs float32 [n, 6] (min, max) ->
        (bins_xyz, counts uint32 [bins], indices uint32 [bins, cap])."""
        aabbs = np.ascontiguousarray(aabbs, dtype=np.float32).reshape(-1, 6)
        keep = []
        d = lb.desc(aabbs.shape[0], keep)
        ts = max(lb.tile_size, 1)
        bx, by = (lb.width + ts - 1) // ts, (lb.height + ts - 1) // ts
        n_bins = bx * by * (max(lb.z_slices, 1) if lb.mode == 3 else 1)
        counts = np.zeros(n_bins, np.uint32)
        idx = np.zeros((n_bins, d.max_per_bin), np.uint32)
        bins = np.zeros(3, np.uint32)
        self._check(self._lib.shs_light_bin_culling(self._h, ctypes.byref(d), aabbs.ctypes.data, aabbs.shape[0],
                                                    bins.ctypes.data, counts.ctypes.data, idx.ctypes.data))
        return tuple(int(b) for b in bins), counts, idx

    def lib_timing_reset(self):
        self._check(self._lib.shs_lib_timing_reset(self._h))

    def lib_timing_read(self):
        """-> ({shadow, camera} pass counts, {kernel: mean ms}) since lib_timing_reset()."""
        s = (ctypes.c_double * 4)()
        n = (ctypes.c_int64 * 2)()
        self._check(self._lib.shs_lib_timing_read(self._h, s, n))
        ns, nc = max(n[0], 1), max(n[1], 1)
        return {"shadow": n[0], "camera": n[1]}, {"shadow_setup": s[0] / ns, "shadow_raster": s[1] / ns,
                                                    "setup": s[2] / nc, "raster": s[3] / nc}

    def lib_stats(self) -> dict:
        from ._abi import LibStats
        s = LibStats()
        self._check(self._lib.shs_get_lib_stats(self._h, ctypes.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in LibStats._fields_}

    @property
    def stream(self):
        return self._lib.shs_get_stream(self._h)


def _is_device(a):
    return hasattr(a, "is_cuda") and a.is_cuda


def _empty_like(a):
    if _is_device(a):
        import torch
        return torch.empty_like(a)
    return np.empty_like(a)


def _host_c(a, dtype):
    return a if _is_device(a) else np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    if _is_device(a):
        assert a.is_contiguous()
        return ctypes.c_void_p(a.data_ptr())
    assert a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.c_void_p)
