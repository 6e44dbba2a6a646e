"""tests/canvas_rt_motion_ref (ref_canvas_rt_motion.c), the C restatement of the unclipped camera pass that
hello_multi_pass.cpp, hello_camera_and_perobject_motion_blur.cpp and hello_glowing_star.cpp share -- the reference of
tests/test_canvas_rt_motion.py -- pinned on the CPU:

  * against a float32 numpy witness of the whole pass, written from the same cited lines and vectorised per triangle
    (np_render_motion), on every scene of the GPU tests: ids, depth, velocity and spec bit for bit, the colour floats
    within helpers.TOL * 255.  The witness takes pow from the host libm, as the restatement does, and the normal matrix
    from test_sky.np_inverse, the float32 restatement of glm::inverse;
  * by hand-computed known answers: one triangle's coverage, depth and colour at a named pixel, the velocity just
    under and just over the clamp, spec01 at normal incidence;
  * test_scenes_show_their_edges: the witness with one rule of the clipped raster swapped in at a time changes pixels
    on the scene built for that rule, so a kernel that kept the clipped raster's behaviour cannot pass.

It also holds what fails without the feature and needs no GPU: the library's new entry points and the ctypes structs
against the header's sizes."""
import ctypes
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
import test_sky as SK
from test_canvas_rt_ref import F, FLT_MAX, H, NEAR_M, W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_motion_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_motion_ref.so")
_P = ctypes.c_void_p
PX_ZTIE, PX_CLAMPED = 4, 8
BAR = helpers.TOL * 255.0
EYE = np.eye(4, dtype=F).reshape(16)


class MotionPlanes(ctypes.Structure):
    _fields_ = [("color", _P), ("depth", _P), ("velocity", _P), ("prequant", _P), ("tri_id", _P), ("spec", _P), ("flags", _P),
                ("counters", ctypes.c_int64 * 4)]


@functools.lru_cache(maxsize=None)
def ref_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    L.rcm_render.restype = ctypes.c_int
    L.rcm_render.argtypes = [ctypes.POINTER(R.RefFrame), ctypes.c_int32, ctypes.POINTER(R.RefDraw), ctypes.c_int, ctypes.POINTER(MotionPlanes)]
    L.rcm_velocity.restype = ctypes.c_int
    L.rcm_velocity.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P]
    L.rcm_fragment.restype = None
    L.rcm_fragment.argtypes = [ctypes.c_int32, _P, _P, _P, _P, _P, _P, _P]
    return L


def ref_render_motion(frame, draws):
    """The pass of a shs_gpu.RtFrame with shading 6 or 7 -> the planes (canvas rows) and counters."""
    Wd, Hd = frame.width, frame.height
    keep = []
    arr = R._ref_draws(draws, keep)
    f = R.RefFrame()
    f.W, f.H = Wd, Hd
    f.tile_w, f.tile_h = frame.ref_tile
    for k in range(4):
        f.clear[k] = frame.clear_color[k]
    f.view[:] = [float(v) for v in np.asarray(frame.view, F).reshape(16)]
    f.light_dir[:] = [float(v) for v in frame.light_dir_world]
    f.camera_pos[:] = [float(v) for v in frame.camera_pos]
    f.max_velocity_px = frame.max_velocity_px
    out = {"color": np.empty((Hd, Wd, 4), np.uint8), "depth": np.empty((Hd, Wd), F), "velocity": np.empty((Hd, Wd, 2), F),
           "prequant": np.empty((Hd, Wd, 4), F), "tri_id": np.empty((Hd, Wd), np.int32), "spec": np.empty((Hd, Wd), F),
           "flags": np.empty((Hd, Wd), np.int32)}
    p = MotionPlanes()
    for k, v in out.items():
        setattr(p, k, v.ctypes.data)
    assert ref_lib().rcm_render(ctypes.byref(f), frame.shading, arr, len(draws), ctypes.byref(p)) == 0
    out["counters"] = dict(zip(("input_tris", "polys3", "polys4", "sub_tris"), (int(c) for c in p.counters)))
    return out


# ---- scenes (shared with tests/test_canvas_rt_motion.py) -------------------------------------------------------

def motion_frame(view, shading, cam_pos=R.CAM_POS, light_dir=R.LIGHT_DIR, w=W, h=H, tile=(80, 80), max_velocity_px=40.0):
    import shs_gpu
    return shs_gpu.RtFrame(w, h, np.asarray(view, F), EYE, tuple(float(F(v)) for v in light_dir), tuple(float(F(v)) for v in cam_pos),
                           ref_tile=tile, max_velocity_px=max_velocity_px, use_shadow=False, pcf=False, prequant=True, shading=shading)


def clip_draw(mesh, prev=None, color=(210, 180, 90, 255), mvp=NEAR_M):
    """A draw whose positions are clip-space x, y and clip z: clip = (x, y, z, z + 1) under NEAR_M, view z = z."""
    import shs_gpu
    return shs_gpu.RtDraw(mesh, EYE, np.asarray(mvp, F), np.asarray(mvp if prev is None else prev, F), color)


def star_prism(R_out=1.0, r_in=0.5, thick=0.5, peak=0.3):
    """A ten-point ring extruded to a prism with a raised centre on both caps: 40 flat-shaded triangles, closed, every
    triangle wound so that cross(b - a, c - a) points outward (what this raster draws when it faces the camera)."""
    ang = np.radians(90.0) + np.arange(10) * np.radians(36.0)
    rad = np.where(np.arange(10) % 2 == 0, R_out, r_in)
    ring = np.stack([np.cos(ang) * rad, np.sin(ang) * rad], 1)
    tris = []
    for i in range(10):
        j = (i + 1) % 10
        a0, a1 = (*ring[i], -0.5 * thick), (*ring[j], -0.5 * thick)
        b0, b1 = (*ring[i], 0.5 * thick), (*ring[j], 0.5 * thick)
        tris += [((0, 0, -0.5 * thick - peak), a0, a1), ((0, 0, 0.5 * thick + peak), b1, b0), (a0, b0, b1), (a0, b1, a1)]
    pos, nrm = [], []
    for t in np.asarray(tris, np.float64):
        n = np.cross(t[1] - t[0], t[2] - t[0])
        if np.dot(n, t.mean(0)) < 0:            # the prism is star-shaped about the origin
            t, n = t[[0, 2, 1]], -n
        pos.append(t.reshape(9))
        nrm.append(np.tile(n / np.linalg.norm(n), 3))
    return R.SoupMesh(np.array(pos, F), np.array(nrm, F))


def scene_demo6(w=W, h=H, tile=(80, 80)):
    """hello_multi_pass.cpp in miniature: three monkeys, one turning slowly, one that moved far (its velocity is clamped at
    40 px), one at rest.  968 triangles each: the records cross the raster's rounds of 256."""
    from shs_gpu import scene
    view, proj = R.camera(w, h)
    s = (1.8, 1.8, 1.8)
    draws = [R._rt_draw(scene.monkey(), scene.model_trs((-3.5, 1.5, 3.0), 20.0, s), view, proj,
                        prev_model=scene.model_trs((-3.5, 1.5, 3.0), 8.0, s), color=(60, 100, 200, 255)),
             R._rt_draw(scene.monkey(), scene.model_trs((0.0, 1.2, 1.0), -30.0, s), view, proj,
                        prev_model=scene.model_trs((5.5, 1.2, 1.0), -30.0, s), color=(200, 90, 80, 255)),
             R._rt_draw(scene.monkey(), scene.model_trs((3.5, 1.8, 4.5), 200.0, s), view, proj, color=(80, 200, 120, 255))]
    return motion_frame(view, 6, w=w, h=h, tile=tile, max_velocity_px=40.0), draws


STAR_CAM = (0.0, 0.5, -2.3)


def scene_demo7(w=W, h=H):
    """hello_glowing_star.cpp in miniature: the star turning, one job covering the frame, max velocity 30.  The light is
    placed so that the facet that faces the camera most mirrors it into the camera at one of the facet's corners: spec01 is
    clamped at 1 there, falls through (0, 1) across that facet and its neighbours, and is exactly 0 (powf underflows) further
    round."""
    from shs_gpu import scene
    view, proj = R.camera(w, h, pos=STAR_CAM, target=(0.0, 0.5, 0.0))
    mesh = star_prism()
    model = scene.model_trs((0.0, 0.5, 0.0), 25.0, (1.0, 1.0, 1.0))
    m = np.asarray(model, np.float64).reshape(4, 4).T
    tri = mesh.positions.astype(np.float64).reshape(-1, 3, 3) @ m[:3, :3].T + m[:3, 3]
    nrm = mesh.normals.astype(np.float64).reshape(-1, 3, 3)[:, 0] @ np.linalg.inv(m[:3, :3])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tocam = np.asarray(STAR_CAM) - tri.mean(1)
    tocam /= np.linalg.norm(tocam, axis=1, keepdims=True)
    k = int(np.argmax((nrm * tocam).sum(1)))
    at = np.asarray(STAR_CAM) - tri[k][1]                               # the mirror direction is exact at one corner
    at /= np.linalg.norm(at)
    ldir = 2.0 * np.dot(nrm[k], at) * nrm[k] - at                       # towards the light
    draws = [R._rt_draw(mesh, model, view, proj, prev_model=scene.model_trs((0.15, 0.5, 0.0), 13.0, (1.0, 1.0, 1.0)),
                        color=(240, 200, 60, 255))]
    return motion_frame(view, 7, cam_pos=STAR_CAM, light_dir=-ldir, w=w, h=h, tile=(w, h), max_velocity_px=30.0), draws


def scene_windings():
    """A quad this raster draws and, nearer, its copy in the other winding, which shows nothing."""
    view, proj = R.camera()
    draws = [R._rt_draw(R.quad_xy(-3.0, 2.0, 0.5, 4.0, 6.0, flip=True), EYE, view, proj, color=(220, 60, 60, 255)),
             R._rt_draw(R.quad_xy(-1.0, 4.0, 1.5, 5.0, 4.5), EYE, view, proj, color=(60, 60, 220, 255))]
    return motion_frame(view, 6), draws


def behind_mesh():
    nan = float("nan")
    tris = [[-0.5, -0.5, 0.5, 0.5, -0.5, 0.5, 0.0, 0.3, -1.5],      # 0: a corner at w = -0.5: drawn, mirrored
            [0.5, -0.8, 0.5, 0.7, -0.3, -1.0, 0.9, -0.8, 0.5],      # 1: a corner at w = 0: Inf / NaN on the screen
            [0.2, 0.3, 0.5, nan, 0.8, 0.5, 0.8, 0.3, 0.5],          # 2: a NaN corner
            [-1.35, 0.3, 0.5, -0.9, 1.2, 0.5, -0.45, 0.3, 0.5],     # 3: a zero normal: NaN colour floats, bytes 0
            [0.3, 0.6, 0.2, 0.75, 1.3, 0.2, 1.2, 0.6, 0.2]]         # 4: an ordinary triangle
    nrm = np.tile(np.array([0, 0, -1] * 3, F), (len(tris), 1))
    nrm[3] = 0
    return R.SoupMesh(np.array(tris, F), nrm)


def scene_behind(shading=6):
    prev = NEAR_M.copy()
    prev[12] = 0.03
    return motion_frame(EYE, shading, cam_pos=(0.0, 0.0, -3.0)), [clip_draw(behind_mesh(), prev)]


def scene_coincident():
    """The same triangle twice in two draws of different colours: the first of equal depths wins."""
    T = [-0.6, -0.6, 0.6, -0.1, 0.7, 0.8, 0.5, -0.5, 0.3]
    n = np.array([[0, 0, -1] * 3], F)
    return motion_frame(EYE, 6, cam_pos=(0.0, 0.0, -3.0)), [clip_draw(R.SoupMesh(np.array([T], F), n), color=(230, 40, 40, 255)),
                                                            clip_draw(R.SoupMesh(np.array([T], F), n), color=(40, 40, 230, 255))]


def scene_hair():
    """test_canvas_rt_ref.hair_soup's slivers under tile jobs of (48, 56), which cut 160 x 120 unevenly: the tile-clamp visit set."""
    mesh = R.hair_soup(np.random.default_rng(99), W, H, R.HAIR_N)
    return motion_frame(EYE, 6, cam_pos=(0.0, 0.0, -3.0), tile=(48, 56)), [clip_draw(mesh, mvp=EYE, color=(200, 120, 40, 255))]


def ndc_quad(x0, x1, y0, y1, z):
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return R.SoupMesh(np.array([np.concatenate([a, c, b]), np.concatenate([a, d, c])], F), np.tile(np.array([0, 0, -1] * 3, F), (2, 1)))


def scene_tiny_motion():
    """max_velocity_px = 0 and a motion of about 5e-5 px: len > 0 holds and len > 0.0001 does not, so the velocity is kept."""
    prev = EYE.copy()
    prev[12] = -5e-5 / (0.5 * (W - 1))
    return motion_frame(EYE, 6, cam_pos=(0.0, 0.0, -3.0), max_velocity_px=0.0), [clip_draw(ndc_quad(-0.6, 0.5, -0.5, 0.6, 0.4), prev, mvp=EYE)]


def scene_prev_behind():
    """The previous clip w runs through zero across the first quad (prev w = z - 0.2 over z in [0, 0.5]) and is zero
    everywhere on the second (a prev_mvp whose w row is zero): Inf and NaN velocities."""
    n = np.tile(np.array([0, 0, -1] * 3, F), (2, 1))
    a, b, c, d = (-0.9, -0.6, 0.0), (0.0, -0.6, 0.5), (0.0, 0.5, 0.5), (-0.9, 0.5, 0.0)
    tilted = R.SoupMesh(np.array([np.concatenate([a, c, b]), np.concatenate([a, d, c])], F), n)
    p0 = NEAR_M.copy()
    p0[15] = -0.2
    p1 = NEAR_M.copy()
    p1[3] = p1[7] = p1[11] = p1[15] = 0.0
    return motion_frame(EYE, 6, cam_pos=(0.0, 0.0, -3.0)), [clip_draw(tilted, p0), clip_draw(ndc_quad(0.2, 1.2, -0.5, 0.6, 0.4), p1, (90, 200, 90, 255))]


SCENES = {"demo6": scene_demo6, "demo7": scene_demo7, "windings": scene_windings, "behind": scene_behind,
          "behind_star": lambda: scene_behind(7), "coincident": scene_coincident, "hair": scene_hair, "tiny_motion": scene_tiny_motion,
          "prev_behind": scene_prev_behind, "97x61": lambda: scene_demo6(97, 61), "160x1": lambda: scene_demo6(160, 1),
          "1x120": lambda: scene_demo6(1, 120), "star_97x61": lambda: scene_demo7(97, 61)}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def scene_ref(name):
    """The restatement's planes of a scene, computed once and shared (read only)."""
    frame, draws = scene(name)
    return ref_render_motion(frame, draws)


# ---- what fails without the feature, without a GPU -------------------------------------------------------------

def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in ("shs_rt_render_motion", "shs_rt_resolve_spec", "shs_rt_device_spec"):
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_ctypes_structs_have_the_headers_sizes(tmp_path):
    """shs_rt_frame is reused as it is: no struct changed size, and the header declares the new entries."""
    from shs_gpu import _abi
    # the header declares the three entries with these signatures (compiled, not linked)
    decl = tmp_path / "decl.c"
    decl.write_text('#include "shs_gpu.h"\nint (*f)(shs_ctx *, const shs_rt_frame *, const shs_rt_draw *, int32_t) = shs_rt_render_motion;\n'
                    'int (*g)(shs_ctx *, float *) = shs_rt_resolve_spec;\nint (*h)(shs_ctx *, void **) = shs_rt_device_spec;\n')
    subprocess.run(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "decl.o"), str(decl)], check=True)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) { printf("%zu %zu\\n", sizeof(shs_rt_frame), sizeof(shs_rt_draw)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_abi.RtFrameC), ctypes.sizeof(_abi.RtDrawC)] == [192, 204]


# ---- the numpy witness ------------------------------------------------------------------------------------------

_libm = ctypes.CDLL("libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def _powf(x, e):
    return np.array([_libm.powf(float(v), e) for v in np.asarray(x, F).reshape(-1)], F).reshape(np.shape(x))


def _gmin(x, y):
    return y if y < x else x


def _gmax(x, y):
    return y if x < y else x


def _m4(m, P_):
    """mat4 * vec4(p, 1) over points [..., 3] -> [..., 4], GLM's sum order."""
    m = np.asarray(m, F)
    x, y, z = P_[..., 0], P_[..., 1], P_[..., 2]
    return np.stack([(m[r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r] * F(1)) for r in range(4)], -1)


def _norm3(v):
    d = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
    return v * (F(1) / np.sqrt(d))[..., None]


def _mix(u, v, w, a, b, c):
    """bc.x * a + bc.y * b + bc.z * c from the left; a, b, c scalars or vectors of the corners."""
    if np.ndim(a) == 0:
        return (u * a + v * b) + w * c
    return (u[:, None] * a + v[:, None] * b) + w[:, None] * c


SWAPS = ("back_faces", "persp_world", "invw_rule", "vel_1e-6", "clipped_area_rule")


def np_render_motion(frame, draws, swap=None):
    """The whole pass in float32 numpy: per tile job and triangle, the pixels of the clamped bbox at once.  swap: one rule
    of the clipped raster in place of this raster's (SWAPS)."""
    Wd, Hd = frame.width, frame.height
    tw, th = min(frame.ref_tile[0], Wd), min(frame.ref_tile[1], Hd)
    star = frame.shading == 7
    depth = np.full((Hd, Wd), FLT_MAX, F)
    ids = np.full((Hd, Wd), -1, np.int32)
    vel = np.zeros((Hd, Wd, 2), F)
    spec = np.zeros((Hd, Wd), F)
    pq = np.zeros((Hd, Wd, 4), F)
    kept = 0
    vmin = F(1e-6) if swap == "vel_1e-6" else F(0.0001)
    L = _norm3(-np.asarray(frame.light_dir_world, F))
    cam = np.asarray(frame.camera_pos, F)
    maxv = F(frame.max_velocity_px)

    def screen(p):
        return ((p[..., 0] / p[..., 3] + F(1)) * F(0.5)) * F(Wd - 1), ((F(1) - p[..., 1] / p[..., 3]) * F(0.5)) * F(Hd - 1)

    with np.errstate(all="ignore"):
        vs, base = [], 0
        for d in draws:
            pos = np.asarray(d.mesh.positions, F).reshape(-1, 3, 3)
            nrm = np.asarray(d.mesh.normals, F).reshape(-1, 3, 3)
            inv = SK.np_inverse(d.model)
            n3 = [inv[r * 4 + c] for c in range(3) for r in range(3)]          # mat3(transpose(inverse(model))), column-major
            n = np.stack([n3[0 + r] * nrm[..., 0] + n3[3 + r] * nrm[..., 1] + n3[6 + r] * nrm[..., 2] for r in range(3)], -1)
            clip = _m4(d.mvp, pos)
            sx, sy = screen(clip)
            vs.append(dict(clip=clip, prev=_m4(d.prev_mvp, pos), world=_m4(d.model, pos)[..., :3], n=_norm3(n),
                           vz=_m4(R._mul(frame.view, d.model), pos)[..., 2], sx=sx, sy=sy, base=base,
                           col=np.array(d.base_color[:3], F) / F(255)))
            base += pos.shape[0]
        first = True
        for ty in range((Hd + th - 1) // th):
            for tx in range((Wd + tw - 1) // tw):
                tminx, tminy = F(tx * tw), F(ty * th)
                tmaxx, tmaxy = F(min((tx + 1) * tw, Wd) - 1), F(min((ty + 1) * th, Hd) - 1)
                for v in vs:
                    for k in range(v["sx"].shape[0]):
                        sx, sy = v["sx"][k], v["sy"][k]
                        bx0, by0, bx1, by1 = tmaxx, tmaxy, tminx, tminy
                        for i in range(3):
                            bx0, by0 = _gmax(tminx, _gmin(bx0, sx[i])), _gmax(tminy, _gmin(by0, sy[i]))
                            bx1, by1 = _gmin(tmaxx, _gmax(bx1, sx[i])), _gmin(tmaxy, _gmax(by1, sy[i]))
                        v0x, v0y, v1x, v1y = sx[1] - sx[0], sy[1] - sy[0], sx[2] - sx[0], sy[2] - sy[0]
                        area = v0x * v1y - v0y * v1x
                        if swap == "back_faces":
                            culled = bool(area == 0)
                        elif swap == "clipped_area_rule":
                            culled = bool(abs(area) < F(1e-8))
                        else:
                            culled = bool(area <= 0)
                        if first and not culled:
                            kept += 1
                        if bx0 > bx1 or by0 > by1 or culled:
                            continue
                        d00, d01, d11 = v0x * v0x + v0y * v0y, v0x * v1x + v0y * v1y, v1x * v1x + v1y * v1y
                        den = d00 * d11 - d01 * d01
                        if abs(float(den)) < 1e-5:
                            continue
                        xs, ys = np.arange(int(bx0), int(bx1) + 1), np.arange(int(by0), int(by1) + 1)
                        vpx = ((xs.astype(F) + F(0.5)) - sx[0])[None, :]
                        vpy = ((ys.astype(F) + F(0.5)) - sy[0])[:, None]
                        d20, d21 = vpx * v0x + vpy * v0y, vpx * v1x + vpy * v1y
                        bv = (d11 * d20 - d01 * d21) / den
                        bw = (d00 * d21 - d01 * d20) / den
                        bu = F(1) - bv - bw
                        vz = v["vz"][k]
                        z = (bu * vz[0] + bv * vz[1]) + bw * vz[2]
                        cy = Hd - 1 - ys
                        win = ~((bu < 0) | (bv < 0) | (bw < 0)) & (z < depth[np.ix_(cy, xs)])
                        if not win.any():
                            continue
                        iy, ix = np.nonzero(win)
                        oy, ox = cy[iy], xs[ix]
                        u, b, w = bu[iy, ix], bv[iy, ix], bw[iy, ix]
                        depth[oy, ox] = z[iy, ix]
                        clip, prev = v["clip"][k], v["prev"][k]
                        if swap in ("invw_rule", "persp_world"):
                            iw = np.array([F(0) if abs(c[3]) < F(1e-6) else F(1) / c[3] for c in clip], F)
                            isum = _mix(u, b, w, iw[0], iw[1], iw[2])
                        if swap == "invw_rule":
                            show = ~(isum <= F(1e-8))
                            oy, ox, u, b, w = oy[show], ox[show], u[show], b[show], w[show]
                        N = _norm3(_norm3(_mix(u, b, w, *v["n"][k])))
                        if swap == "persp_world":
                            wp = v["world"][k]
                            world = _mix(u, b, w, wp[0] * iw[0], wp[1] * iw[1], wp[2] * iw[2]) / isum[:, None]
                        else:
                            world = _mix(u, b, w, *v["world"][k])
                        csx, csy = screen(_mix(u, b, w, *clip))
                        psx, psy = screen(_mix(u, b, w, *prev))
                        vx, vy = csx - psx, -(csy - psy)
                        ln = np.sqrt(vx * vx + vy * vy)
                        cl = (ln > maxv) & (ln > vmin)
                        s = np.where(cl, maxv / ln, F(1))
                        vel[oy, ox, 0], vel[oy, ox, 1] = np.where(cl, vx * s, vx), np.where(cl, vy * s, vy)
                        V = _norm3(cam - world)
                        dot = lambda a, c: (a[..., 0] * c[..., 0] + a[..., 1] * c[..., 1]) + a[..., 2] * c[..., 2]   # noqa: E731
                        ndl = dot(N, L)
                        diffuse = np.where(ndl < 0, F(0), ndl)
                        ndh = dot(N, _norm3(L + V))
                        ndh = np.where(ndh < 0, F(0), ndh)
                        col = v["col"]
                        if star:
                            s01 = F(3.85) * _powf(ndh, 256.0)
                            s01 = np.where(s01 < 0, F(0), np.where(s01 > 1, F(1), s01))
                            lit = F(0.20) + diffuse
                            res = lit[:, None] * (col * F(0.85))[None, :] + s01[:, None] * np.array([1.0, 0.90, 0.55], F)[None, :]
                            spec[oy, ox] = s01
                            pq[oy, ox, 3] = s01
                        else:
                            lit = (F(0.35) + diffuse) + F(0.5) * _powf(ndh, 64.0)
                            res = lit[:, None] * col[None, :]
                            pq[oy, ox, 3] = 1
                        res = np.where(res < 0, F(0), res)
                        res = np.where(F(1) < res, F(1), res)
                        pq[oy, ox, :3] = res * F(255)
                        ids[oy, ox] = 2 * (v["base"] + k)
                first = False
    return dict(depth=depth, tri_id=ids, velocity=vel, spec=spec, prequant=pq, kept=kept)


def _bits(a):
    return P.canonical_bits(a)


def assert_witness(ref, wit, label):
    assert np.array_equal(ref["tri_id"], wit["tri_id"]), f"{label}: ids"
    for k in ("depth", "velocity", "spec"):
        bad = np.argwhere(_bits(ref[k]) != _bits(wit[k]))
        assert bad.size == 0, f"{label}: {len(bad)} {k} words differ, first {bad[:3].tolist()}"
    a, b = ref["prequant"], wit["prequant"]
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{label}: NaN colour floats on one side only"
    dp = np.nan_to_num(np.abs(a[..., :3] - b[..., :3]), nan=0.0)
    assert dp.max() <= BAR, f"{label}: colour floats differ by {dp.max()}"
    assert ref["counters"]["sub_tris"] == wit["kept"]


@pytest.mark.parametrize("name", list(SCENES))
def test_restatement_equals_numpy_witness(name):
    frame, draws = scene(name)
    assert_witness(scene_ref(name), np_render_motion(frame, draws), name)


# ---- known answers ------------------------------------------------------------------------------------------------

def test_one_triangle_known_answer():
    """A right triangle with screen corners A (10.25, 10.25), B (30.25, 10.25), C (10.25, 30.25) on a 41 x 41 frame (screen =
    (ndc + 1) * 20, y down), w = 1, view z = clip z = 0.25 / 0.5 / 0.75, facing the camera and the light head-on from far
    away.  No pixel centre lies on an edge: the pixels shown are x, y >= 10 with x + y <= 39, 210 of them.  At pixel
    (15, 15), centre (15.5, 15.5): v = w = 5.25 / 20 = 0.2625, u = 0.475, depth 0.475 * 0.25 + 0.2625 * 0.5 + 0.2625 * 0.75 =
    0.446875.  N . L = 1 and N . H = 1: lit = 0.35 + 1 + 0.5 = 1.85; for colour (101, 50, 7): 1.85 * 101 = 186.85 -> 186,
    1.85 * 50 = 92.5 -> 92, 1.85 * 7 = 12.95 -> 12."""
    import shs_gpu
    sx = lambda px: px / 20.0 - 1.0      # noqa: E731
    sy = lambda py: 1.0 - py / 20.0      # noqa: E731
    tri = [sx(10.25), sy(10.25), 0.25, sx(30.25), sy(10.25), 0.5, sx(10.25), sy(30.25), 0.75]
    mesh = R.SoupMesh(np.array([tri], F), np.array([[0, 0, -1] * 3], F))
    draws = [shs_gpu.RtDraw(mesh, EYE, EYE, EYE, (101, 50, 7, 255))]
    frame = motion_frame(EYE, 6, cam_pos=(0.0, 0.0, -1e6), light_dir=(0.0, 0.0, 1.0), w=41, h=41, tile=(41, 41))
    out = ref_render_motion(frame, draws)
    shown = out["tri_id"][::-1] == 0                                   # screen rows
    ys, xs = np.mgrid[0:41, 0:41]
    assert np.array_equal(shown, (xs >= 10) & (ys >= 10) & (xs + ys <= 39)) and shown.sum() == 210
    assert abs(out["depth"][40 - 15, 15] - 0.446875) < 1e-6
    assert tuple(out["color"][40 - 15, 15]) == (186, 92, 12, 255)
    assert out["prequant"][40 - 15, 15, 3] == 1.0 and out["counters"] == {"input_tris": 1, "polys3": 0, "polys4": 0, "sub_tris": 1}
    # the other winding shows nothing
    back = [shs_gpu.RtDraw(R.SoupMesh(np.array([tri], F).reshape(1, 3, 3)[:, [0, 2, 1]].reshape(1, 9), np.array([[0, 0, -1] * 3], F)), EYE, EYE, EYE)]
    out = ref_render_motion(frame, back)
    assert (out["tri_id"] == -1).all() and out["counters"]["sub_tris"] == 0


def test_velocity_clamp_known_answers():
    L = ref_lib()
    out = np.zeros(2, F)

    def vel(dx_px, max_px, w=101):
        cur = np.array([0.0, 0.0, 0.5, 1.0], F)
        prv = np.array([-dx_px / (0.5 * (w - 1)), 0.0, 0.5, 1.0], F)
        c = L.rcm_velocity(cur.ctypes.data, prv.ctypes.data, w, 51, max_px, out.ctypes.data)
        return out.copy(), c
    assert abs(vel(29.5, 30.0)[0][0] - 29.5) < 1e-5 and vel(29.5, 30.0)[1] == 0  # just under: kept
    v, c = vel(30.5, 30.0)
    assert c == 1 and abs(v[0] - 30.0) < 1e-5 and v[1] == 0.0                    # just over: scaled onto the limit
    assert abs(vel(-80.0, 40.0)[0][0] + 40.0) < 1e-5
    # the second threshold: with a limit of 0, a length of 5e-5 is kept and one of 2e-4 becomes 0
    v, c = vel(5e-5, 0.0, w=3)                                                   # (w = 3: one ndc unit is one pixel)
    assert c == 0 and abs(v[0] - 5e-5) < 1e-6
    v, c = vel(2e-4, 0.0, w=3)
    assert c == 1 and v[0] == 0.0


def test_fragment_known_answers():
    """Normal incidence: N = L = V, so N . H = 1 and spec = 1.  Shading 7: spec01 = clampf(3.85, 0, 1) = 1 and the byte is
    255 * min(1, (0.20 + 1) * 0.85 * c + tint): c = 40 / 255 gives 0.16 + tint -> (255, 255, 181) for tints (1, 0.90, 0.55).
    With the light and the camera both in the surface's plane N . L = N . H = 0: the star's colour is 0.2 * 0.85 * c and
    spec01 = 3.85 * pow(0, 256) = 0.  Shading 6 at normal incidence: (0.35 + 1 + 0.5) * c.  (The colours keep every product
    away from a whole number, where the truncation would hang on the last bit.)"""
    L = ref_lib()
    pre, rgba = np.zeros(4, F), np.zeros(4, np.uint8)

    def frag(shading, light, cam, color, normal=(0, 0, -1), world=(0, 0, 0)):
        a = [np.array(v, t) for v, t in ((light, F), (cam, F), (color, np.uint8), (normal, F), (world, F))]
        L.rcm_fragment(shading, *(x.ctypes.data for x in a), pre.ctypes.data, rgba.ctypes.data)
        return pre.copy(), tuple(int(v) for v in rgba)
    p, c = frag(7, (0, 0, 1), (0, 0, -5), (40, 40, 40, 255))
    assert p[3] == 1.0 and c == (255, 255, int(255 * (1.2 * 0.85 * 40 / 255 + 0.55)), 255) and c[2] == 181
    p, c = frag(7, (1, 0, 0), (-5, 0, 0), (201, 101, 52, 255))
    assert p[3] == 0.0 and c == (34, 17, 8, 255)                      # 0.17 * (201, 101, 52) = 34.17, 17.17, 8.84
    p, c = frag(6, (0, 0, 1), (0, 0, -5), (101, 50, 7, 255))
    assert p[3] == 1.0 and c == (186, 92, 12, 255)
    # clampf passes a NaN on: a zero normal gives NaN spec01 and NaN colour floats, bytes 0
    p, c = frag(7, (0, 0, 1), (0, 0, -5), (40, 40, 40, 255), normal=(0, 0, 0))
    assert np.isnan(p).all() and c == (0, 0, 0, 255)


# ---- the scenes show what they are there for ------------------------------------------------------------------------

def test_scenes_cover_what_the_gpu_tests_need():
    out = scene_ref("demo6")
    shown = out["tri_id"] >= 0
    ln = np.hypot(out["velocity"][..., 0], out["velocity"][..., 1])
    cl = (out["flags"] & PX_CLAMPED) != 0
    assert shown.sum() > 1500 and cl.sum() > 300 and (shown & ~cl & (ln > 0.5)).sum() > 300 and (shown & (ln == 0)).sum() > 300
    assert np.abs(ln[cl] - 40.0).max() < 1e-3 and out["counters"]["input_tris"] > 3 * 256
    per = scene("demo6")[1][0].mesh.positions.shape[0]
    assert len(set((out["tri_id"][shown] // 2 // per).tolist())) == 3 and (out["tri_id"][shown] % 2 == 0).all()
    assert 0 < out["counters"]["sub_tris"] < out["counters"]["input_tris"] and out["counters"]["polys3"] == out["counters"]["polys4"] == 0

    out = scene_ref("demo7")
    shown = out["tri_id"] >= 0
    s = out["spec"]
    assert shown.sum() > 2000 and (s[shown] == 0).sum() > 100 and ((s > 0) & (s < 1)).sum() > 100 and (s == 1).sum() > 20
    assert ((s > 0.05) & (s < 0.95)).sum() > 20 and not s[~shown].any()
    assert np.array_equal(_bits(s), _bits(out["prequant"][..., 3]))

    out = scene_ref("windings")
    assert set(np.unique(out["tri_id"])) == {-1, 0, 2} and out["counters"]["sub_tris"] == 2

    out = scene_ref("behind")
    ids = out["tri_id"]
    assert set(np.unique(ids)) == {-1, 0, 6, 8} and (ids == 0).sum() > 300
    assert np.isnan(out["prequant"][ids == 6][:, :3]).all() and (out["color"][ids == 6][:, :3] == 0).all()
    assert out["depth"][ids == 0].min() < 0            # the mirrored corner's view z is negative and interpolates in
    st = scene_ref("behind_star")
    assert np.isnan(st["spec"][st["tri_id"] == 6]).all() and not np.isnan(st["spec"][st["tri_id"] != 6]).any()

    out = scene_ref("coincident")
    assert set(np.unique(out["tri_id"])) == {-1, 0} and ((out["flags"] & PX_ZTIE) != 0).sum() > 500 and out["counters"]["sub_tris"] == 2

    frame, draws = scene("hair")
    out = scene_ref("hair")
    one = ref_render_motion(dataclasses.replace(frame, ref_tile=(W, H)), draws)
    assert not np.array_equal(out["depth"].view(np.uint32), one["depth"].view(np.uint32))   # the tile clamp changes the image

    out = scene_ref("tiny_motion")
    ln = np.hypot(out["velocity"][..., 0], out["velocity"][..., 1])[out["tri_id"] >= 0]
    assert ((ln > 0) & (ln < 1e-4)).sum() > 1000 and ln.max() < 1e-4

    out = scene_ref("prev_behind")
    v = out["velocity"]
    assert np.isnan(v[out["tri_id"] >= 4]).any() and np.isfinite(v[(out["tri_id"] >= 0) & (out["tri_id"] < 4)]).any()
    assert (np.abs(v[np.isfinite(v)]) <= 40.001).all()

    assert (scene_ref("160x1")["tri_id"] == -1).all()      # H - 1 = 0: every screen y is 0, every area 0
    assert (scene_ref("97x61")["tri_id"] >= 0).sum() > 500


@pytest.mark.parametrize("swap,name", [("back_faces", "windings"), ("persp_world", "demo6"), ("invw_rule", "behind"), ("vel_1e-6", "tiny_motion"),
                                       ("clipped_area_rule", "windings")])
def test_scenes_show_their_edges(swap, name):
    """The witness with one rule of the clipped raster swapped in changes pixels on the scene built for it: another
    triangle shown, a colour float moved by more than the bar, or a velocity word changed.  (The two area rules differ in
    what they keep of the back faces; a positive area under 1e-8 px^2, which they also treat differently, has a denom near
    area^2 < 1e-5 and draws nothing either way.)"""
    frame, draws = scene(name)
    ref = scene_ref(name)
    wit = np_render_motion(frame, draws, swap)
    moved = (ref["tri_id"] != wit["tri_id"]) | (_bits(ref["velocity"]) != _bits(wit["velocity"])).any(-1)
    with np.errstate(invalid="ignore"):
        moved |= (np.nan_to_num(np.abs(ref["prequant"][..., :3] - wit["prequant"][..., :3]), nan=0.0) > BAR).any(-1)
    assert moved.sum() > 50, f"{swap} on {name}: {int(moved.sum())} pixels changed"
