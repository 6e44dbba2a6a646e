"""tests/canvas_rt_ref (ref_canvas_rt.c), the C restatement of the Canvas render-target raster of
hello-render-target/hello_shadow_mapping.cpp -- the reference of tests/test_canvas_rt.py -- pinned on the CPU:

  * against the oracle's legacy raster: with an orthographic mvp (w = 1) and view z set to NDC z an unclipped
    triangle's coverage and depth are the legacy pipeline's (same clip_to_screen, barycentric_coordinate,
    tile clamp and strict '<'), once the corners are pre-rotated to undo the clip loop's {v1, v2, v0} order;
  * against a float32 numpy restatement written from the same cited lines, per pixel, on a clipped quad and
    a clipped triangle (depth, shading sub-triangle, velocity, texel);
  * by known answers: the clip loop's outputs, shadow_compare / the PCF at their edges, the velocity clamp;
  * and the scenes of the GPU tests are checked to show, in the reference's output, what they are there for.

It also holds what fails without the feature and needs no GPU: the library's new entry points, shs_ortho_lh_zo
against the restatement, and the ctypes structs against the header's sizes."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers
from test_legacy_texture_ref import coded_texture, texel_of_prequant  # noqa: F401  (the GPU tests take them from here)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_ref.so")
F = np.float32
FLT_MAX = helpers.FLT_MAX
_P = ctypes.c_void_p
_F16 = ctypes.c_float * 16
PX_SUV_OUTSIDE, PX_NEG_AREA, PX_ZTIE = 1, 2, 4


class RefDraw(ctypes.Structure):
    _fields_ = [("positions", _P), ("normals", _P), ("uvs", _P), ("n_tris", ctypes.c_int32), ("model", _F16), ("mvp", _F16),
                ("prev_mvp", _F16), ("base_color", ctypes.c_uint8 * 4), ("texels", _P), ("tw", ctypes.c_int32),
                ("th", ctypes.c_int32)]


class RefFrame(ctypes.Structure):
    _fields_ = [("W", ctypes.c_int32), ("H", ctypes.c_int32), ("tile_w", ctypes.c_int32), ("tile_h", ctypes.c_int32),
                ("clear", ctypes.c_uint8 * 4), ("view", _F16), ("light_vp", _F16), ("light_dir", ctypes.c_float * 3),
                ("camera_pos", ctypes.c_float * 3), ("bias_base", ctypes.c_float), ("bias_slope", ctypes.c_float),
                ("max_velocity_px", ctypes.c_float), ("pcf", ctypes.c_int32), ("shadow", _P), ("sw", ctypes.c_int32),
                ("sh", ctypes.c_int32)]


class RefPlanes(ctypes.Structure):
    _fields_ = [("color", _P), ("depth", _P), ("velocity", _P), ("prequant", _P), ("tri_id", _P), ("texel", _P),
                ("flags", _P), ("counters", ctypes.c_int64 * 4)]


@functools.lru_cache(maxsize=None)
def ref_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    L.rcr_render_shadow.restype = ctypes.c_int
    L.rcr_render_shadow.argtypes = [ctypes.c_int] * 4 + [_P, ctypes.POINTER(RefDraw), ctypes.c_int, _P]
    L.rcr_render.restype = ctypes.c_int
    L.rcr_render.argtypes = [ctypes.POINTER(RefFrame), ctypes.POINTER(RefDraw), ctypes.c_int, ctypes.POINTER(RefPlanes)]
    L.rcr_ortho_lh_zo.restype = None
    L.rcr_ortho_lh_zo.argtypes = [ctypes.c_float] * 6 + [_P]
    L.rcr_clip.restype = ctypes.c_int
    L.rcr_clip.argtypes = [_P, _P, _P]
    for fn in (L.rcr_shadow_compare, L.rcr_shadow_pcf):
        fn.restype = ctypes.c_float
        fn.argtypes = [_P, ctypes.c_int, ctypes.c_int] + [ctypes.c_float] * 4
    L.rcr_velocity.restype = None
    L.rcr_velocity.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P]
    return L


def _ref_draws(draws, keep):
    arr = (RefDraw * max(len(draws), 1))()
    for i, d in enumerate(draws):
        pos = np.ascontiguousarray(d.mesh.positions, F)
        nrm = np.ascontiguousarray(d.mesh.normals, F)
        uvs = None if getattr(d.mesh, "uvs", None) is None else np.ascontiguousarray(d.mesh.uvs, F)
        keep += [pos, nrm, uvs]
        arr[i].positions, arr[i].normals = pos.ctypes.data, nrm.ctypes.data
        arr[i].uvs = None if uvs is None else uvs.ctypes.data
        arr[i].n_tris = pos.shape[0]
        eye = np.eye(4, dtype=F).reshape(16)
        for name in ("model", "mvp", "prev_mvp"):
            m = getattr(d, name)
            getattr(arr[i], name)[:] = [float(v) for v in (eye if m is None else np.asarray(m, F).reshape(16))]
        for k in range(4):
            arr[i].base_color[k] = d.base_color[k]
        if d.albedo_tex is not None:
            t = np.ascontiguousarray(d.albedo_tex.rgba, np.uint8)
            keep.append(t)
            arr[i].texels, arr[i].tw, arr[i].th = t.ctypes.data, t.shape[1], t.shape[0]
    return arr


def ref_shadow(size, light_vp, casters, tile=(80, 80)):
    """PASS0 -> the shadow map float32 [h, w] (y down)."""
    w, h = (size, size) if isinstance(size, int) else size
    keep = []
    arr = _ref_draws(casters, keep)
    lvp = np.ascontiguousarray(light_vp, F).reshape(16)
    sm = np.empty((h, w), F)
    assert ref_lib().rcr_render_shadow(w, h, tile[0], tile[1], lvp.ctypes.data, arr, len(casters), sm.ctypes.data) == 0
    return sm


def ref_render(frame, draws, shadow=None):
    """PASS1 of a shs_gpu.RtFrame -> the planes (canvas rows) and counters."""
    W, H = frame.width, frame.height
    keep = []
    arr = _ref_draws(draws, keep)
    f = RefFrame()
    f.W, f.H = W, H
    f.tile_w, f.tile_h = frame.ref_tile
    for k in range(4):
        f.clear[k] = frame.clear_color[k]
    f.view[:] = [float(v) for v in np.asarray(frame.view, F).reshape(16)]
    f.light_vp[:] = [float(v) for v in np.asarray(frame.light_vp, F).reshape(16)]
    f.light_dir[:] = [float(v) for v in frame.light_dir_world]
    f.camera_pos[:] = [float(v) for v in frame.camera_pos]
    f.bias_base, f.bias_slope, f.max_velocity_px, f.pcf = frame.bias_base, frame.bias_slope, frame.max_velocity_px, int(frame.pcf)
    if frame.use_shadow:
        assert shadow is not None
        sm = np.ascontiguousarray(shadow, F)
        f.shadow, f.sw, f.sh = sm.ctypes.data, sm.shape[1], sm.shape[0]
    out = {"color": np.empty((H, W, 4), np.uint8), "depth": np.empty((H, W), F), "velocity": np.empty((H, W, 2), F),
           "prequant": np.empty((H, W, 4), F), "tri_id": np.empty((H, W), np.int32), "texel": np.empty((H, W), np.int32),
           "flags": np.empty((H, W), np.int32)}
    p = RefPlanes()
    for k, v in out.items():
        setattr(p, k, v.ctypes.data)
    assert ref_lib().rcr_render(ctypes.byref(f), arr, len(draws), ctypes.byref(p)) == 0
    out["counters"] = dict(zip(("input_tris", "polys3", "polys4", "sub_tris"), (int(c) for c in p.counters)))
    return out


# ---- scenes (shared with tests/test_canvas_rt.py) --------------------------------------------------------

class SoupMesh:
    def __init__(self, positions, normals=None, uvs=None):
        self.positions = np.ascontiguousarray(positions, F).reshape(-1, 9)
        self.normals = np.tile(np.array([0, 1, 0] * 3, F), (self.positions.shape[0], 1)) if normals is None else \
            np.ascontiguousarray(normals, F).reshape(-1, 9)
        self.uvs = None if uvs is None else np.ascontiguousarray(uvs, F).reshape(-1, 6)


def _mul(a, b):
    from shs_gpu import scene
    return scene.mat_mul(a, b)


def floor_grid(cells=6, x0=-12.0, x1=12.0, z0=-20.0, z1=28.0):
    """A cells x cells grid in y = 0; with the camera at z = -9 its near rows reach behind the camera."""
    xs, zs = np.linspace(x0, x1, cells + 1), np.linspace(z0, z1, cells + 1)
    tris = []
    for j in range(cells):
        for i in range(cells):
            a, b, c, d = (xs[i], 0, zs[j]), (xs[i + 1], 0, zs[j]), (xs[i + 1], 0, zs[j + 1]), (xs[i], 0, zs[j + 1])
            tris += [np.concatenate([a, c, b]), np.concatenate([a, d, c])]
    return SoupMesh(np.array(tris, F))


def quad_xy(x0, x1, y0, y1, z, uv0=-0.25, uv1=1.25, flip=False):
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    ua, ub, uc, ud = (uv0, uv0), (uv1, uv0), (uv1, uv1), (uv0, uv1)
    if flip:
        pos = [np.concatenate([a, c, b]), np.concatenate([a, d, c])]
        uv = [np.concatenate([ua, uc, ub]), np.concatenate([ua, ud, uc])]
    else:
        pos = [np.concatenate([a, b, c]), np.concatenate([a, c, d])]
        uv = [np.concatenate([ua, ub, uc]), np.concatenate([ua, uc, ud])]
    return SoupMesh(np.array(pos, F), np.tile(np.array([0, 0, -1] * 3, F), (2, 1)), np.array(uv, F))


W, H, SM = 160, 120, 96
CAM_POS = (0.0, 4.0, -9.0)
LIGHT_DIR = (-0.45, -1.0, 0.55)
TEX = coded_texture(16, 12, 10, 5, 10, 7)


def camera(w=W, h=H, pos=CAM_POS, target=(0.0, 0.5, 0.0)):
    from shs_gpu import lib_path
    view = lib_path.look_at_lh(pos, target)
    proj = lib_path.perspective_lh_no(float(np.radians(60.0)), w / h, 0.1, 100.0)
    return view, proj


def ortho_lh_zo(l, r, b, t, zn, zf):
    from shs_gpu import _abi
    out = np.zeros(16, F)
    assert _abi.lib().shs_ortho_lh_zo(l, r, b, t, zn, zf, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
    return out


def light(center=(0.0, 0.0, 2.0), dist=20.0, ext=9.0, zn=0.1, zf=40.0):
    """The demo's light camera (:1305-1317): look_at from center - dir * dist, ortho_lh_zo."""
    from shs_gpu import lib_path
    d = np.asarray(LIGHT_DIR, np.float64)
    d = d / np.linalg.norm(d)
    eye = tuple(float(v) for v in np.asarray(center) - d * dist)
    return _mul(ortho_lh_zo(-ext, ext, -ext, ext, zn, zf), lib_path.look_at_lh(eye, center))


def _rt_draw(mesh, model, view, proj, prev_model=None, color=(200, 200, 200, 255), tex=None):
    import shs_gpu
    vp = _mul(proj, view)
    return shs_gpu.RtDraw(mesh, np.asarray(model, F), _mul(vp, model), _mul(vp, model if prev_model is None else prev_model),
                          color, tex)


def _frame(view, light_vp, w=W, h=H, tile=(80, 80), **kw):
    import shs_gpu
    return shs_gpu.RtFrame(w, h, view, light_vp, LIGHT_DIR, CAM_POS, ref_tile=tile, prequant=True, **kw)


def scene_demo(light_kw=None):
    """The demo in miniature: the floor reaching behind the camera, the spinning monkey over it, a textured quad."""
    from shs_gpu import scene
    view, proj = camera()
    eye = np.eye(4, dtype=F).reshape(16)
    draws = [
        _rt_draw(floor_grid(), eye, view, proj, color=(120, 160, 120, 255)),
        _rt_draw(scene.monkey(), scene.model_trs((-1.0, 2.2, 2.0), 20.0, (1.6, 1.6, 1.6)), view, proj,
                 prev_model=scene.model_trs((-1.0, 2.2, 2.0), 8.0, (1.6, 1.6, 1.6)), color=(200, 140, 60, 255)),
        _rt_draw(quad_xy(2.0, 6.0, 0.3, 4.3, 5.0), eye, view, proj, tex=TEX),
    ]
    return view, light(**(light_kw or {})), draws


def scene_windings():
    """The same quad in each winding, the reversed one nearer: nothing may be culled."""
    view, proj = camera()
    eye = np.eye(4, dtype=F).reshape(16)
    draws = [_rt_draw(quad_xy(-3.0, 2.0, 0.5, 4.0, 6.0), eye, view, proj, color=(220, 60, 60, 255)),
             _rt_draw(quad_xy(-1.0, 4.0, 1.5, 5.0, 4.5, flip=True), eye, view, proj, color=(60, 60, 220, 255)),
             _rt_draw(quad_xy(-6.0, -2.5, 0.0, 3.0, 5.0, flip=True), eye, view, proj, color=(60, 220, 60, 255))]
    return view, light(), draws


# clip = (x, y, z, z + 1): z is the clip z, so a corner at z = 0 lies exactly on the plane and w stays near 1
NEAR_M = np.eye(4, dtype=F)
NEAR_M[3, 2] = 1.0
NEAR_M = np.ascontiguousarray(NEAR_M.T).reshape(16)   # column-major: m[2 * 4 + 3] = 1


def near_mesh():
    tris = [
        [-0.9, -0.8, 0.5, -0.3, -0.8, 0.5, -0.6, -0.2, -0.4],      # one corner behind
        [0.1, -0.8, -0.3, 0.7, -0.8, -0.4, 0.4, -0.1, 0.6],        # two corners behind
        [-0.9, 0.2, -0.2, -0.5, 0.2, -0.3, -0.7, 0.7, -0.1],       # all behind: nothing
        [-0.3, 0.1, 0.0, 0.3, 0.1, 0.4, 0.0, 0.8, 0.3],            # a corner exactly on z = 0
        [0.4, 0.2, 0.0, 0.9, 0.2, -5e-9, 0.65, 0.8, 0.5],          # bz - az below 1e-8: t = 0
        [-0.2, -0.6, 0.7, 0.1, -0.9, 0.2, 0.3, -0.5, 0.9],         # unclipped
    ]
    uv = np.tile(np.array([0, 0, 1, 0, 0.5, 1], F), (len(tris), 1))
    return SoupMesh(np.array(tris, F), np.tile(np.array([0, 0, -1] * 3, F), (len(tris), 1)), uv)


def scene_near():
    import shs_gpu
    eye = np.eye(4, dtype=F).reshape(16)
    prev = NEAR_M.copy()
    prev[12] = 0.03   # the previous frame: shifted in x
    draws = [shs_gpu.RtDraw(near_mesh(), eye, NEAR_M, prev, (210, 180, 90, 255), TEX)]
    return eye, light(center=(0.0, 0.0, 0.5), dist=5.0, ext=1.5, zf=12.0), draws


def scene_coincident():
    """T (unclipped) and S (one corner behind: two sub-triangles) drawn twice in different draws and colours, in
    the other order the second time: ids 0, 2, 3 | 4, 5, 6.  The first of equal depths wins, so 4 .. 6 show nowhere."""
    import shs_gpu
    eye = np.eye(4, dtype=F).reshape(16)
    T = [-0.6, -0.6, 0.6, 0.5, -0.5, 0.3, -0.1, 0.7, 0.8]
    S = [-0.8, 0.1, 0.5, 0.6, -0.2, 0.7, 0.1, 0.9, -0.5]
    n = np.tile(np.array([0, 0, -1] * 3, F), (2, 1))
    draws = [shs_gpu.RtDraw(SoupMesh(np.array([T, S], F), n), eye, NEAR_M, NEAR_M, (230, 40, 40, 255)),
             shs_gpu.RtDraw(SoupMesh(np.array([S, T], F), n), eye, NEAR_M, NEAR_M, (40, 40, 230, 255))]
    return eye, light(center=(0.0, 0.0, 0.5), dist=5.0, ext=1.5, zf=12.0), draws


def scene_outside_light():
    """A light whose box is smaller than the scene in x / y and in depth: receivers outside its extent and range,
    casters that partly leave the map and partly have z outside [0, 1]."""
    return scene_demo(dict(center=(-1.0, 1.0, 2.0), dist=6.0, ext=3.0, zn=3.5, zf=7.5))


def hair_soup(rng, w, h, n):
    """tests/test_gpu_parity.py's _hair_soup (slivers whose third vertex lies within 0.02 px of the long edge), with
    z in (0, 1): inside the shadow pass's range and in front of the camera pass's clip plane."""
    tris = []
    for _ in range(n):
        c = rng.uniform([0, 0], [w, h])
        d = rng.normal(size=2); d /= np.linalg.norm(d)
        L = rng.uniform(20, 400)
        nrm = np.array([-d[1], d[0]])
        p = np.stack([c, c + d * L, c + d * L * rng.uniform(0.05, 0.95) + nrm * rng.uniform(-0.02, 0.02)])
        z = rng.uniform(0.05, 0.9, size=3)
        x = p[:, 0] / (0.5 * (w - 1)) - 1.0
        y = 1.0 - p[:, 1] / (0.5 * (h - 1))
        tris.append(np.stack([x, y, z], axis=1).reshape(9))
    pos = np.asarray(tris, dtype=F)
    return SoupMesh(pos, rng.normal(size=pos.shape).astype(F))


HAIR_W, HAIR_H, HAIR_N = 400, 300, 1500


def scene_hair():
    import shs_gpu
    eye = np.eye(4, dtype=F).reshape(16)
    mesh = hair_soup(np.random.default_rng(99), HAIR_W, HAIR_H, HAIR_N)
    return eye, eye, [shs_gpu.RtDraw(mesh, eye, eye, eye, (200, 120, 40, 255))]


def render_both_ref(view, light_vp, draws, w=W, h=H, sm=SM, tile=(80, 80), **kw):
    """Both passes through the restatement -> (shadow map, camera planes)."""
    shadow = ref_shadow(sm, light_vp, draws, tile)
    return shadow, ref_render(_frame(view, light_vp, w, h, tile, **kw), draws, shadow)


# ---- what fails without the feature, without a GPU ---------------------------------------------------------

NEW_ENTRY_POINTS = ["shs_rt_render_shadow", "shs_rt_render", "shs_rt_resolve", "shs_rt_resolve_shadow", "shs_rt_resolve_prequant",
                    "shs_rt_resolve_ids", "shs_rt_get_stats", "shs_rt_device_targets", "shs_ortho_lh_zo"]


def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in NEW_ENTRY_POINTS:
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_ortho_lh_zo_equals_the_restatement_bitwise():
    rng = np.random.default_rng(3)
    cases = [(-28.0, 28.0, -28.0, 28.0, 0.1, 200.0)] + [tuple(float(F(v)) for v in rng.uniform(-50, 50, 6)) for _ in range(20)]
    for c in cases:
        want = np.zeros(16, F)
        ref_lib().rcr_ortho_lh_zo(*c, want.ctypes.data)
        got = ortho_lh_zo(*c)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), c
    m = ortho_lh_zo(-2.0, 2.0, -1.0, 1.0, 1.0, 5.0)
    assert m[0] == 0.5 and m[5] == 1.0 and m[10] == 0.25 and m[14] == -0.25 and m[15] == 1.0 and m[12] == 0.0


def test_ctypes_structs_have_the_headers_sizes(tmp_path):
    from shs_gpu import _abi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(shs_rt_draw), '
                   'sizeof(shs_rt_frame), sizeof(shs_rt_stats)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_abi.RtDrawC), ctypes.sizeof(_abi.RtFrameC), ctypes.sizeof(_abi.RtStatsC)]


# ---- the restatement against the oracle's legacy raster ------------------------------------------------------

def test_orthographic_frame_is_the_legacy_rasters(oracle_mod):
    """w = 1 and view z = NDC z: depth (and so coverage) equals the legacy pipeline's on unclipped triangles."""
    import shs_gpu
    from shs_gpu.scene import Mesh
    rng = np.random.default_rng(5)
    w, h, n = 96, 72, 60
    px = rng.uniform([-5, -5], [w + 5, h + 5], size=(n, 1, 2)) + rng.uniform(-20, 20, size=(n, 3, 2))
    v0, v1 = px[:, 1] - px[:, 0], px[:, 2] - px[:, 0]
    flip = (v0[:, 0] * v1[:, 1] - v0[:, 1] * v1[:, 0]) <= 0      # the legacy raster draws positive screen area only
    px[flip] = px[flip][:, [0, 2, 1]]
    pos = np.empty((n, 3, 3), F)
    pos[..., 0] = px[..., 0] / (0.5 * (w - 1)) - 1.0
    pos[..., 1] = 1.0 - px[..., 1] / (0.5 * (h - 1))
    pos[..., 2] = rng.uniform(0.05, 0.9, size=(n, 3))
    nrm = rng.normal(size=(n, 9)).astype(F)
    eye = np.eye(4, dtype=F).reshape(16)
    legacy = shs_gpu.Draw(Mesh(pos.reshape(n, 9), nrm), 3, eye, eye, np.array([-0.3, -0.5, 0.8], F), np.array([0, 0, -3], F))
    _, ref_d, _ = oracle_mod.render_legacy(w, h, [legacy], tile=(80, 80))
    rot = pos[:, [2, 0, 1]].reshape(n, 9)                         # {c, a, b} leaves the clip loop as {a, b, c}
    mine = shs_gpu.RtDraw(SoupMesh(rot, nrm.reshape(n, 3, 3)[:, [2, 0, 1]].reshape(n, 9)), eye, eye, eye)
    out = ref_render(shs_gpu.RtFrame(w, h, eye, eye, LIGHT_DIR, CAM_POS, use_shadow=False), [mine])
    assert (ref_d < FLT_MAX).sum() > 500
    helpers.assert_depth_bitexact(out["depth"][::-1], ref_d)      # canvas rows against the legacy screen rows
    assert out["counters"] == {"input_tris": n, "polys3": n, "polys4": 0, "sub_tris": n}


# ---- the restatement against numpy --------------------------------------------------------------------------

def _m4(m, p):
    m = np.asarray(m, F)
    x, y, z = (F(v) for v in p)
    return [F(F(F(m[r] * x) + F(m[4 + r] * y)) + F(F(m[8 + r] * z) + F(m[12 + r] * F(1)))) for r in range(4)]


def _np_clip(vs):
    """clip_poly_near_z (:877-913) over dicts of float32 arrays."""
    def inside(v):
        return v["p"][3] > F(1e-6) and v["p"][2] >= F(0)

    def cut(a, b):
        az, bz = a["p"][2], b["p"][2]
        den = F(bz - az)
        t = F(0) if abs(den) < F(1e-8) else F(F(F(0) - az) / den)
        t = F(0) if t < 0 else (F(1) if t > 1 else t)
        return {k: np.array([F(x + F(F(y - x) * t)) for x, y in zip(a[k], b[k])], F) for k in a}
    out = []
    for i in range(3):
        A, B = vs[i], vs[(i + 1) % 3]
        if inside(A) and inside(B):
            out.append(B)
        elif inside(A):
            out.append(cut(A, B))
        elif inside(B):
            out += [cut(A, B), B]
    return out


def np_render(frame, draws):
    """Depth, sub-triangle, velocity and texel per pixel in float32 numpy, one tile job (the bbox is the frame)."""
    Wd, Hd = frame.width, frame.height
    depth = np.full((Hd, Wd), FLT_MAX, F)
    ids = np.full((Hd, Wd), -1, np.int32)
    vel = np.zeros((Hd, Wd, 2), F)
    texel = np.full((Hd, Wd), -1, np.int32)
    t = 0

    def screen(p):
        return F(F(F(F(p[0] / p[3]) + F(1)) * F(0.5)) * F(Wd - 1)), F(F(F(F(1) - F(p[1] / p[3])) * F(0.5)) * F(Hd - 1))
    with np.errstate(all="ignore"):
        for d in draws:
            vm = _mul(frame.view, d.model)
            for k in range(d.mesh.positions.shape[0]):
                vs = []
                for c in range(3):
                    p = d.mesh.positions[k, 3 * c:3 * c + 3]
                    uv = d.mesh.uvs[k, 2 * c:2 * c + 2] if d.mesh.uvs is not None else np.zeros(2, F)
                    vs.append({"p": np.array(_m4(d.mvp, p), F), "q": np.array(_m4(d.prev_mvp, p), F), "uv": np.array(uv, F),
                               "vz": np.array([_m4(vm, p)[2]], F)})
                poly = _np_clip(vs)
                for ti in range(1, len(poly) - 1):
                    tv = [poly[0], poly[ti], poly[ti + 1]]
                    if any(v["p"][3] <= F(1e-6) for v in tv):
                        continue
                    s = [screen(v["p"]) for v in tv]
                    v0 = (F(s[1][0] - s[0][0]), F(s[1][1] - s[0][1]))
                    v1 = (F(s[2][0] - s[0][0]), F(s[2][1] - s[0][1]))
                    area = F(F(v0[0] * v1[1]) - F(v0[1] * v1[0]))
                    if abs(area) < F(1e-8):
                        continue
                    d00 = F(F(v0[0] * v0[0]) + F(v0[1] * v0[1]))
                    d01 = F(F(v0[0] * v1[0]) + F(v0[1] * v1[1]))
                    d11 = F(F(v1[0] * v1[0]) + F(v1[1] * v1[1]))
                    den = F(F(d00 * d11) - F(d01 * d01))
                    if abs(float(den)) < 1e-5:
                        continue
                    clampx = lambda v: min(max(v, F(0)), F(Wd - 1))
                    clampy = lambda v: min(max(v, F(0)), F(Hd - 1))
                    x0, x1 = int(clampx(min(p[0] for p in s))), int(clampx(max(p[0] for p in s)))
                    y0, y1 = int(clampy(min(p[1] for p in s))), int(clampy(max(p[1] for p in s)))
                    iw = [F(0) if abs(v["p"][3]) < F(1e-6) else F(F(1) / v["p"][3]) for v in tv]
                    for py in range(y0, y1 + 1):
                        for px in range(x0, x1 + 1):
                            vx, vy = F(F(px + 0.5) - s[0][0]), F(F(py + 0.5) - s[0][1])
                            d20 = F(F(vx * v0[0]) + F(vy * v0[1]))
                            d21 = F(F(vx * v1[0]) + F(vy * v1[1]))
                            bv = F(F(F(d11 * d20) - F(d01 * d21)) / den)
                            bw = F(F(F(d00 * d21) - F(d01 * d20)) / den)
                            bu = F(F(F(1) - bv) - bw)
                            if bu < 0 or bv < 0 or bw < 0:
                                continue

                            def mix(a, b, c):
                                return F(F(F(bu * a) + F(bv * b)) + F(bw * c))
                            vz = mix(tv[0]["vz"][0], tv[1]["vz"][0], tv[2]["vz"][0])
                            yc = Hd - 1 - py
                            if not vz < depth[yc, px]:
                                continue
                            depth[yc, px] = vz
                            isum = mix(iw[0], iw[1], iw[2])
                            if isum <= F(1e-8):
                                continue
                            pos = [mix(tv[0]["p"][j], tv[1]["p"][j], tv[2]["p"][j]) for j in range(4)]
                            prv = [mix(tv[0]["q"][j], tv[1]["q"][j], tv[2]["q"][j]) for j in range(4)]
                            cs, ps = screen(pos), screen(prv)
                            v = np.array([F(cs[0] - ps[0]), -F(cs[1] - ps[1])], F)
                            ln = np.sqrt(F(F(v[0] * v[0]) + F(v[1] * v[1])))
                            if ln > F(frame.max_velocity_px) and ln > F(1e-6):
                                v = (v * F(F(frame.max_velocity_px) / ln)).astype(F)
                            vel[yc, px] = v
                            ids[yc, px] = 2 * t + ti - 1
                            if d.albedo_tex is not None:
                                th, tw = d.albedo_tex.rgba.shape[:2]
                                uvx = F(mix(F(tv[0]["uv"][0] * iw[0]), F(tv[1]["uv"][0] * iw[1]), F(tv[2]["uv"][0] * iw[2])) / isum)
                                uvy = F(mix(F(tv[0]["uv"][1] * iw[0]), F(tv[1]["uv"][1] * iw[1]), F(tv[2]["uv"][1] * iw[2])) / isum)
                                sx = F(min(max(uvx, F(0)), F(1)) * F(tw - 1))
                                sy = F(min(max(uvy, F(0)), F(1)) * F(th - 1))
                                texel[yc, px] = int(np.floor(float(sy) + 0.5)) * tw + int(np.floor(float(sx) + 0.5))
                t += 1
    return depth, ids, vel, texel


def test_raster_equals_numpy_restatement():
    """A clipped quad (one corner behind) and a clipped triangle (two behind), textured, moving."""
    import shs_gpu
    eye = np.eye(4, dtype=F).reshape(16)
    prev = NEAR_M.copy()
    prev[12] = 0.15   # 3.5 / w px on a 48 x 36 frame: the clamp at 3 px acts near w = 1 only
    mesh = SoupMesh(near_mesh().positions[:2], near_mesh().normals[:2], near_mesh().uvs[:2])
    draws = [shs_gpu.RtDraw(mesh, eye, NEAR_M, prev, (210, 180, 90, 255), TEX)]
    frame = shs_gpu.RtFrame(48, 36, eye, eye, LIGHT_DIR, CAM_POS, ref_tile=(48, 36), use_shadow=False, max_velocity_px=3.0)
    out = ref_render(frame, draws)
    assert out["counters"] == {"input_tris": 2, "polys3": 1, "polys4": 1, "sub_tris": 3}
    depth, ids, vel, texel = np_render(frame, draws)
    assert set(np.unique(ids)) == {-1, 0, 1, 2}
    helpers.assert_depth_bitexact(out["depth"], depth)
    assert np.array_equal(out["tri_id"], ids)
    assert np.array_equal(out["velocity"].view(np.uint32), vel.view(np.uint32))
    assert np.array_equal(out["texel"], texel)
    ln = np.hypot(out["velocity"][..., 0], out["velocity"][..., 1])
    assert (np.abs(ln[ids >= 0] - 3.0) < 1e-5).any() and (ln[ids >= 0] < 2.9).any()


# ---- known answers ----------------------------------------------------------------------------------------------

def _clip(tri):
    pos = np.ascontiguousarray(tri, F).reshape(12)
    out, vz = np.zeros(16, F), np.zeros(4, F)
    n = ref_lib().rcr_clip(pos.ctypes.data, out.ctypes.data, vz.ctypes.data)
    return n, out.reshape(4, 4)[:n], vz[:n]


def test_clip_known_answers():
    # unclipped: the loop pushes B, so {v0, v1, v2} leaves as {v1, v2, v0} (view z 1, 2, 3 -> 2, 3, 1)
    n, p, vz = _clip([[0, 0, 0.5, 1], [1, 0, 0.5, 1], [0, 1, 0.5, 1]])
    assert n == 3 and list(vz) == [2, 3, 1]
    # a corner exactly on z = 0 is inside
    n, p, vz = _clip([[0, 0, 0.0, 1], [1, 0, 0.5, 1], [0, 1, 0.5, 1]])
    assert n == 3 and list(vz) == [2, 3, 1]
    # all behind (z < 0, or w <= 1e-6): nothing
    assert _clip([[0, 0, -0.1, 1], [1, 0, -0.5, 1], [0, 1, -1, 1]])[0] == 0
    assert _clip([[0, 0, 0.5, 1e-6], [1, 0, 0.5, 0.0], [0, 1, 0.5, -1]])[0] == 0
    # v2 behind: v0 -> v1 pushes v1, v1 -> v2 the cut at t = 0.5 / 1.5, v2 -> v0 the cut at t = 2 / 3 and v0
    n, p, vz = _clip([[0, 0, 1.0, 1], [2, 0, 0.5, 1], [0, 2, -1.0, 1]])
    t1, t2 = F(F(0.0) - F(0.5)) / F(F(-1.0) - F(0.5)), F(F(0.0) - F(-1.0)) / F(F(1.0) - F(-1.0))
    assert n == 4 and vz[0] == 2 and vz[3] == 1
    assert vz[1] == F(F(2) + F(F(3) - F(2)) * t1) and vz[2] == F(F(3) + F(F(1) - F(3)) * t2)
    assert p[1][0] == F(F(2) + F(F(0) - F(2)) * t1) and p[2][1] == F(F(2) + F(F(0) - F(2)) * t2)
    # bz - az below 1e-8: t = 0, the cut is A itself
    n, p, vz = _clip([[0, 0, 0.0, 1], [1, 0, -5e-9, 1], [0, 1, 0.5, 1]])
    assert n == 4 and vz[0] == 1 and np.array_equal(p[0], np.array([0, 0, 0, 1], F))


def test_shadow_lookup_known_answers():
    L = ref_lib()
    sm = np.full((4, 5), 0.5, F)      # h = 4, w = 5
    sm[0, 0], sm[3, 4], sm[1, 2] = 0.2, 0.9, FLT_MAX
    a = sm.ctypes.data
    cmp_ = lambda u, v, z, b=0.0: L.rcr_shadow_compare(a, 5, 4, u, v, z, b)
    pcf = lambda u, v, z, b=0.0: L.rcr_shadow_pcf(a, 5, 4, u, v, z, b)
    assert cmp_(0.0, 0.0, 0.2) == 1.0 and cmp_(0.0, 0.0, 0.21) == 0.0 and cmp_(0.0, 0.0, 0.21, 0.02) == 1.0
    assert cmp_(1.0, 1.0, 0.9) == 1.0 and cmp_(1.0, 1.0, 0.91) == 0.0
    eps = float(np.nextafter(F(1), F(2)))
    assert cmp_(-1e-7, 0.5, 9.0) == 1.0 and cmp_(eps, 0.5, 9.0) == 1.0 and cmp_(0.5, -1e-7, 9.0) == 1.0   # outside: lit
    assert cmp_(0.5, 1.0 / 3.0, 9.0) == 1.0                       # texel (2, 1) is empty (FLT_MAX): lit
    assert cmp_(0.5, 0.0, 9.0) == 0.0
    # the PCF has no uv check: fx negative clamps to column 0 (x1 = 1), beyond w - 1 to column 4 twice
    assert pcf(-3.0, 0.0, 0.3) == 0.25 * 3                        # (0,0) = 0.2 fails, (1,0), (0,1), (1,1) = 0.5 pass
    assert pcf(7.0, 1.0, 0.7) == 0.25 * 4                         # x0 = x1 = 4, y0 = y1 = 3: 0.9 four times
    assert pcf(7.0, 1.0, 0.95) == 0.0
    assert pcf(0.5, 1.0 / 3.0, 0.6) == 0.25                       # only the empty texel (FLT_MAX + bias) passes
    got = {pcf(0.0, 0.0, z) for z in (0.1, 0.3, 0.6)} | {pcf(0.5, 1.0 / 3.0, 0.6), pcf(0.4, 0.2, 0.3)}
    sm2 = np.array([[0.1, 0.9], [0.9, 0.1]], F)
    vals = {L.rcr_shadow_pcf(sm2.ctypes.data, 2, 2, 0.0, 0.0, z, 0.0) for z in (0.05, 0.5, 0.95)}
    assert vals == {1.0, 0.5, 0.0} and {0.0, 0.25, 0.75, 1.0} <= got | {pcf(-3.0, 0.0, 0.3)}


def test_velocity_clamp_known_answers():
    L = ref_lib()
    out = np.zeros(2, F)

    def vel(dx_px, max_px, w=101):
        cur = np.array([0.0, 0.0, 0.5, 1.0], F)
        prv = np.array([-dx_px / (0.5 * (w - 1)), 0.0, 0.5, 1.0], F)
        L.rcr_velocity(cur.ctypes.data, prv.ctypes.data, w, 51, max_px, out.ctypes.data)
        return out.copy()
    assert vel(10.0, 22.0)[0] == F(10.0) and vel(10.0, 22.0)[1] == 0.0
    assert vel(21.5, 22.0)[0] == F(21.5)                          # just below: kept
    assert abs(vel(22.5, 22.0)[0] - 22.0) < 1e-5                  # just above: scaled onto the limit
    assert abs(vel(-40.0, 22.0)[0] + 22.0) < 1e-5
    cur, prv = np.array([0, 0.5, 0.5, 1], F), np.array([0, 0.0, 0.5, 1], F)
    L.rcr_velocity(cur.ctypes.data, prv.ctypes.data, 101, 51, 22.0, out.ctypes.data)
    assert out[1] == F(12.5) and out[0] == 0.0                    # screen y is down, the canvas velocity up


# ---- the scenes show what they are there for -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene_planes(name, pcf=True, tile=80):
    view, lvp, draws = SCENES[name]()
    return render_both_ref(view, lvp, draws, tile=(tile, tile), pcf=pcf)


SCENES = {"demo": scene_demo, "windings": scene_windings, "near": scene_near, "coincident": scene_coincident,
          "outside": scene_outside_light}


def test_scenes_cover_what_the_gpu_tests_need():
    sm, out = scene_planes("demo")
    c = out["counters"]
    assert c["polys3"] > 0 and c["polys4"] > 0 and c["polys3"] + c["polys4"] < c["input_tris"]
    shaded = out["tri_id"] >= 0
    assert shaded.sum() > 0.5 * W * H and (sm < FLT_MAX).sum() > 500
    assert ((out["tri_id"] & 1) == 1)[shaded].any()                               # a clipped polygon's second sub-triangle shows
    vals = set(np.unique(out["prequant"][..., 3][shaded]).tolist())
    assert vals == {0.0, 0.25, 0.5, 0.75, 1.0}, vals
    assert ((out["flags"] & PX_SUV_OUTSIDE) != 0).sum() > 50
    assert (out["texel"] >= 0).sum() > 200 and len(np.unique(out["texel"])) > 40
    assert np.abs(out["velocity"]).max() > 1.0
    _, nop = scene_planes("demo", pcf=False)
    assert set(np.unique(nop["prequant"][..., 3][nop["tri_id"] >= 0]).tolist()) == {0.0, 1.0}

    _, out = scene_planes("windings")
    neg = (out["flags"] & PX_NEG_AREA) != 0
    assert neg.sum() > 300 and ((out["tri_id"] >= 0) & ~neg).sum() > 300
    assert set(np.unique(out["tri_id"])) == {-1, 0, 2, 4, 6, 8, 10}                # 2 t: every triangle of both windings shows

    _, out = scene_planes("near")
    # one behind: 4 vertices; two behind, on the plane, unclipped: 3; all behind: none; the t = 0 cut: 4, its second
    # sub-triangle {cut = A, C, A} degenerate (area 0: not rastered, id 9 absent)
    assert out["counters"] == {"input_tris": 6, "polys3": 3, "polys4": 2, "sub_tris": 6}
    assert set(np.unique(out["tri_id"])) == {-1, 0, 1, 2, 6, 8, 10}

    _, out = scene_planes("coincident")
    assert (out["flags"] & PX_ZTIE).astype(bool).sum() > 500
    assert set(np.unique(out["tri_id"])) == {-1, 0, 2, 3}
    assert out["counters"]["sub_tris"] == 6

    sm, out = scene_planes("outside")
    shaded = out["tri_id"] >= 0
    assert ((out["flags"] & PX_SUV_OUTSIDE) != 0).sum() > 200
    assert 50 < (sm < FLT_MAX).sum() < 0.9 * SM * SM
    assert (out["prequant"][..., 3][shaded] < 1.0).sum() > 20


def test_hair_slivers_tile_clamp_changes_both_passes():
    """The reference's tile clamp changes the image for these slivers: the 80-tile render differs from the
    single-tile render (as test_hair_slivers_tile_clamp_ghosts checks for the legacy raster)."""
    view, lvp, draws = scene_hair()
    s80 = ref_shadow((HAIR_W, HAIR_H), lvp, draws, (80, 80))
    s1 = ref_shadow((HAIR_W, HAIR_H), lvp, draws, (HAIR_W, HAIR_H))
    assert not np.array_equal(s80.view(np.uint32), s1.view(np.uint32))
    import shs_gpu
    f80 = shs_gpu.RtFrame(HAIR_W, HAIR_H, view, lvp, LIGHT_DIR, CAM_POS, ref_tile=(80, 80), use_shadow=False)
    f1 = shs_gpu.RtFrame(HAIR_W, HAIR_H, view, lvp, LIGHT_DIR, CAM_POS, ref_tile=(HAIR_W, HAIR_H), use_shadow=False)
    d80, d1 = ref_render(f80, draws)["depth"], ref_render(f1, draws)["depth"]
    assert not np.array_equal(d80.view(np.uint32), d1.view(np.uint32))
