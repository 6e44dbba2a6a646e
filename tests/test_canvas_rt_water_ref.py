"""tests/canvas_rt_water_ref (ref_canvas_rt_water.c), the C restatement of hello_water.cpp's camera passes -- the hard demo's
raster with fragment_shader_full (:938-994, the atmosphere shader) and fragment_shader_water (:1000-1097) chosen per draw --
the reference of tests/test_canvas_rt_water.py, pinned on the CPU:

  * against a second restatement of the noise chain and of both shaders in float32 numpy, written from the same cited
    lines: N and foam bit for bit on seeded points (negative coordinates, |x|, |z| up to 1e6, NaN and inf, the times at
    which the blend weight w is exactly 1 and exactly 0, and 1e4), colours within helpers.TOL;
  * by known answers: hash12 at lattice points by hand-ordered float32 operations, the flat normal's foam, the fresnel
    facing the camera and at grazing incidence, a reflection canvas of distinct texels naming (rx, ry_canvas), the shadow
    factor outside the light's uv square where the hard demo's PCF gives another value;
  * against shading 0's restatement: ids, depth and velocity of the same draws are bit-identical;
  * with the ABI structs' sizes and offsets against the ctypes mirror and the new entry points present (these fail
    without the feature and need no GPU);
  * by witnesses: in every scene the GPU test compares, one ulp on one hash12 input moves the colour floats by more than
    100 bars on at least half the water pixels, and where the reflection has distinct texels a lookup one texel off does
    the same on at least half of those that read a texel -- so the GPU comparison cannot hide a wrong normal or texel.

It also holds the wrapper, the scenes and the frames the GPU test shares."""
import ctypes
import dataclasses
import functools
import os
import subprocess
import types

import numpy as np
import pytest

import helpers
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
import test_canvas_rt_skybox_ibl_ref as I
import test_canvas_rt_sky_ref as K
from test_canvas_rt_ref import F, H, SM, W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_water_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_water_ref.so")
_P = ctypes.c_void_p
_F3 = ctypes.c_float * 3
_F16 = ctypes.c_float * 16
BAR = helpers.TOL * 255.0
ATMOSPHERE, REFL_NONE, REFL_W, REFL_OUTSIDE, REFL_TEXEL, NOTHING = -1, 0, 1, 2, 3, -2     # rwt_debug::branch
WITNESS_SHIFT_TEXEL, WITNESS_HASH_ULP = 1, 2
WATER_Y = 0.6
CLEAR_BG = (24, 34, 58, 255)          # hello_water.cpp:86


class RefWater(ctypes.Structure):
    _fields_ = [("reflection_vp", _F16), ("time_sec", ctypes.c_float), ("reflection", _P), ("rw", ctypes.c_int32), ("rh", ctypes.c_int32),
                ("witness", ctypes.c_int32)]


class RefDebug(ctypes.Structure):
    _fields_ = [("normal", _F3), ("foam", ctypes.c_float), ("fresnel", ctypes.c_float), ("rx", ctypes.c_int32), ("ry_canvas", ctypes.c_int32),
                ("branch", ctypes.c_int32), ("suv_outside", ctypes.c_int32), ("shadow", ctypes.c_float)]


class RefDebugPlanes(ctypes.Structure):
    _fields_ = [("normal", _P), ("foam", _P), ("fresnel", _P), ("rxy", _P), ("branch", _P)]


@functools.lru_cache(maxsize=None)
def water_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    L.rwt_render.restype = ctypes.c_int
    L.rwt_render.argtypes = [ctypes.POINTER(R.RefFrame), ctypes.POINTER(RefWater), ctypes.POINTER(R.RefDraw), _P, ctypes.c_int,
                             ctypes.POINTER(R.RefPlanes), ctypes.POINTER(RefDebugPlanes)]
    L.rwt_water_samples.restype = ctypes.c_int
    L.rwt_water_samples.argtypes = [ctypes.c_int, _P, ctypes.c_float, ctypes.c_int, _P, _P]
    L.rwt_fragments.restype = ctypes.c_int
    L.rwt_fragments.argtypes = [ctypes.POINTER(R.RefFrame), ctypes.POINTER(RefWater), ctypes.c_int, _P, _P, _P, _P, _P, _P,
                                ctypes.POINTER(RefDebug)]
    for fn, n in ((L.rwt_hash11, 1), (L.rwt_hash12, 2), (L.rwt_noise2, 2), (L.rwt_fbm2, 2)):
        fn.restype = ctypes.c_float
        fn.argtypes = [ctypes.c_float] * n
    L.rwt_hash22.restype = None
    L.rwt_hash22.argtypes = [ctypes.c_float, _P]
    L.rwt_shadow_factor.restype = ctypes.c_float
    L.rwt_shadow_factor.argtypes = [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_float] * 4
    L.rwt_lround.restype = ctypes.c_int
    L.rwt_lround.argtypes = [ctypes.c_float]
    for fn in (L.rwt_sizeof_water, L.rwt_sizeof_debug):
        fn.restype = ctypes.c_size_t
        fn.argtypes = []
    return L


# ---- the wrapper ------------------------------------------------------------------------------------------------

def _water_c(water, reflection, keep, witness=0):
    w = RefWater()
    vp = np.eye(4, dtype=F).reshape(16) if water.reflection_vp is None else np.asarray(water.reflection_vp, F).reshape(16)
    w.reflection_vp[:] = [float(v) for v in vp]
    w.time_sec = float(water.time_sec)
    w.witness = int(witness)
    if water.reflection:
        assert reflection is not None
        img = np.ascontiguousarray(reflection, np.uint8)
        keep.append(img)
        w.reflection, w.rw, w.rh = img.ctypes.data, img.shape[1], img.shape[0]
    return w


def ref_render_water(frame, draws, surface, water, shadow=None, reflection=None, witness=0):
    """One camera pass of hello_water.cpp for a shs_gpu.RtFrame; surface: one bool per draw; water: a shs_gpu.RtWater;
    reflection: uint8 [h, w, 4] in canvas rows, read when water.reflection -> test_canvas_rt_ref.ref_render's planes and
    counters plus 'normal' [.., 3], 'foam', 'fresnel', 'rxy' [.., 2] and 'branch'."""
    Wd, Hd = frame.width, frame.height
    keep = []
    arr = R._ref_draws(draws, keep)
    f = P._frame_c(frame, shadow, keep)
    wc = _water_c(water, reflection, keep, witness)
    out = {"color": np.empty((Hd, Wd, 4), np.uint8), "depth": np.empty((Hd, Wd), F), "velocity": np.empty((Hd, Wd, 2), F),
           "prequant": np.empty((Hd, Wd, 4), F), "tri_id": np.empty((Hd, Wd), np.int32), "texel": np.empty((Hd, Wd), np.int32),
           "flags": np.empty((Hd, Wd), np.int32)}
    dbg = {"normal": np.empty((Hd, Wd, 3), F), "foam": np.empty((Hd, Wd), F), "fresnel": np.empty((Hd, Wd), F),
           "rxy": np.empty((Hd, Wd, 2), np.int32), "branch": np.empty((Hd, Wd), np.int32)}
    p, g = R.RefPlanes(), RefDebugPlanes()
    for planes, c in ((out, p), (dbg, g)):
        for k, v in planes.items():
            setattr(c, k, v.ctypes.data)
    flags = np.ascontiguousarray([1 if s else 0 for s in surface] or [0], np.int32)
    assert water_lib().rwt_render(ctypes.byref(f), ctypes.byref(wc), arr, flags.ctypes.data, len(draws), ctypes.byref(p), ctypes.byref(g)) == 0
    out.update(dbg)
    out["counters"] = dict(zip(("input_tris", "polys3", "polys4", "sub_tris"), (int(c) for c in p.counters)))
    return out


def ref_water_samples(world, time_sec, witness=0):
    """water_flow_normal_and_foam :862-930 of n points -> (N [n, 3], foam [n])"""
    world = np.ascontiguousarray(world, F).reshape(-1, 3)
    n = world.shape[0]
    nrm, foam = np.empty((n, 3), F), np.empty(n, F)
    assert water_lib().rwt_water_samples(n, world.ctypes.data, float(time_sec), witness, nrm.ctypes.data, foam.ctypes.data) == 0
    return nrm, foam


def ref_fragments(frame, water, surface, normal, world, base, shadow=None, reflection=None):
    """Either shader of n fragments -> (pre [n, 4], rgba [n, 4], debug: a dict of [n, ..] arrays)"""
    keep = []
    f = P._frame_c(frame, shadow, keep)
    wc = _water_c(water, reflection, keep)
    normal, world = np.ascontiguousarray(normal, F).reshape(-1, 3), np.ascontiguousarray(world, F).reshape(-1, 3)
    n = world.shape[0]
    base = np.ascontiguousarray(base, np.uint8).reshape(n, 3)
    surf = np.ascontiguousarray(np.broadcast_to(np.asarray(surface, np.int32), (n,)))
    pre, rgba = np.empty((n, 4), F), np.empty((n, 4), np.uint8)
    dbg = (RefDebug * max(n, 1))()
    assert water_lib().rwt_fragments(ctypes.byref(f), ctypes.byref(wc), n, surf.ctypes.data, normal.ctypes.data, world.ctypes.data,
                                     base.ctypes.data, pre.ctypes.data, rgba.ctypes.data, dbg) == 0
    d = {"normal": np.array([list(g.normal) for g in dbg[:n]], F).reshape(n, 3)}
    for k, t in (("foam", F), ("fresnel", F), ("rx", np.int32), ("ry_canvas", np.int32), ("branch", np.int32), ("suv_outside", np.int32),
                 ("shadow", F)):
        d[k] = np.array([getattr(g, k) for g in dbg[:n]], t)
    return pre, rgba, d


# ---- the scenes (shared with tests/test_canvas_rt_water.py) ------------------------------------------------------------

def water_frame(view, light_vp, cam_pos, w=W, h=H, tile=(80, 80), **kw):
    f = R._frame(view, light_vp, w, h, tile, shading=5, clear_color=CLEAR_BG, **kw)
    return dataclasses.replace(f, camera_pos=tuple(float(v) for v in cam_pos))


def water_grid(cells=4, x0=-14.0, x1=14.0, z0=-7.0, z1=30.0, y=WATER_Y):
    """cells x cells quads in the plane y; larger than the light's box (test_canvas_rt_ref.light: 18 x 18 around (0, 0, 2))."""
    xs, zs = np.linspace(x0, x1, cells + 1), np.linspace(z0, z1, cells + 1)
    tris = []
    for j in range(cells):
        for i in range(cells):
            a, b, c, d = (xs[i], y, zs[j]), (xs[i + 1], y, zs[j]), (xs[i + 1], y, zs[j + 1]), (xs[i], y, zs[j + 1])
            tris += [np.concatenate([a, c, b]), np.concatenate([a, d, c])]
    return R.SoupMesh(np.array(tris, F))


GRAZING_POS, GRAZING_TARGET = (0.5, 1.6, -9.0), (0.0, 0.5, 8.0)


def look(pos, target, up=(0.0, 1.0, 0.0), w=W, h=H, fov=60.0):
    from shs_gpu import lib_path
    view = lib_path.look_at_lh(pos, target, up)
    proj = lib_path.perspective_lh_no(float(np.radians(fov)), w / h, 0.1, 100.0)
    return view, proj


def mirrored(pos, target, w=W, h=H, fov=60.0):
    """compute_reflection_view_lh :1550-1563 -> (view, proj, the mirrored position)"""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    d = (target - pos) / np.linalg.norm(target - pos)
    mpos = np.array([pos[0], 2.0 * WATER_Y - pos[1], pos[2]])
    md = np.array([d[0], -d[1], d[2]])
    view, proj = look(tuple(mpos), tuple(mpos + md), (0.0, -1.0, 0.0), w, h, fov)
    return view, proj, tuple(float(v) for v in mpos)


def objects(view, proj):
    """The floor below the water, the monkey and the textured quad of test_canvas_rt_ref.scene_demo through another camera."""
    from shs_gpu import scene
    eye = np.eye(4, dtype=F).reshape(16)
    return [R._rt_draw(R.floor_grid(), eye, view, proj, color=(120, 160, 120, 255)),
            R._rt_draw(scene.monkey(), scene.model_trs((-1.0, 2.2, 2.0), 20.0, (1.6, 1.6, 1.6)), view, proj,
                       prev_model=scene.model_trs((-1.0, 2.2, 2.0), 8.0, (1.6, 1.6, 1.6)), color=(200, 140, 60, 255)),
            R._rt_draw(R.quad_xy(2.0, 6.0, 0.3, 4.3, 5.0), eye, view, proj, tex=R.TEX)]


def water_draw(view, proj, mesh=None):
    return R._rt_draw(water_grid() if mesh is None else mesh, np.eye(4, dtype=F).reshape(16), view, proj, color=(10, 40, 60, 255))


@functools.lru_cache(maxsize=None)
def distinct_image(w, h, seed=5):
    """A canvas whose every texel is a colour of its own, 17 byte levels apart in some channel (distinct_faces' recipe: 4,096
    colours, so at most that many texels)."""
    levels = np.arange(0, 256, 17)
    pick = np.random.default_rng(seed).choice(len(levels) ** 3, size=w * h, replace=False)
    img = np.full((h, w, 4), 255, np.uint8)
    img[..., :3] = np.stack([levels[pick % 16], levels[(pick // 16) % 16], levels[pick // 256]], -1).reshape(h, w, 3)
    return img


def _f32_times(x):
    return float(F(x) * F(0.18))


@functools.lru_cache(maxsize=None)
def time_with_t0(want):
    """A float32 time_sec whose time = t * 0.18f has fract(time) exactly `want` (0: w = 1; 0.5: w = 0)."""
    for k in range(1, 400):
        t = F((k + want) / 0.18)
        for _ in range(8):
            for c in (t, np.nextafter(t, F(np.inf)), np.nextafter(t, F(-np.inf))):
                p = F(c) * F(0.18)
                if p - np.floor(p) == F(want):
                    return float(c)
            t = np.nextafter(t, F(np.inf))
    raise AssertionError(f"no float32 time with t0 == {want}")


def _nan_vertex(mesh, tri, corner=0):
    pos = mesh.positions.copy()
    pos[tri, 3 * corner] = np.nan
    return R.SoupMesh(pos, mesh.normals, mesh.uvs)


SCENE_NAMES = ("host_reflection", "no_reflection", "outside", "w_tiny", "no_shadow", "compare", "water_first", "water_absent", "two_waters",
               "nan_water", "nan_normal", "nan_atmosphere", "time_w1", "time_w0", "time_1e4", "reflection_1x1", "one_pixel_high", "uneven_tile")


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> a namespace: frame, draws, surface, water (shs_gpu.RtWater), reflection (uint8 [h, w, 4] or None), light_vp, sm, tile.
    Every scene is seen through the grazing camera over a water grid that is larger than the light's box."""
    import shs_gpu
    w, h, sm, tile = W, H, SM, (80, 80)
    if name == "one_pixel_high":
        w, h = 160, 1
    if name == "uneven_tile":
        tile = (64, 48)
    view, proj = look(GRAZING_POS, GRAZING_TARGET, w=w, h=h)
    rview, rproj, _ = mirrored(GRAZING_POS, GRAZING_TARGET, w=w, h=h)
    lvp = R.light(ext=6.0)            # (a light box smaller than the water: uv leaves [0, 1] inside the frame)
    objs = objects(view, proj)
    wd = water_draw(view, proj)
    draws, surface = objs[:1] + [wd] + objs[1:], [False, True, False, False]
    refl = distinct_image(72, 48)
    t = 3.7
    use_shadow, pcf = True, True
    rvp = R._mul(rproj, rview)
    flag = True
    if name == "no_reflection":
        refl, flag = None, False
    elif name == "outside":
        # a narrow mirrored projection: much of the water leaves its rndc square; the water reaches behind that camera
        rview, rproj, _ = mirrored((0.5, 1.6, 4.0), (0.0, 0.5, 21.0), fov=25.0)
        rvp = R._mul(rproj, rview)
    elif name == "w_tiny":
        # clip.w = 1e-7 x: |w| <= 1e-6 for |x| <= 10, and beyond that a quotient far outside the rndc square
        rvp = np.eye(4, dtype=F)
        rvp[:, 3] = 0
        rvp[0, 3] = 1e-7          # column-major storage m[c][r]: row 3 of column 0
        rvp = rvp.reshape(16)
    elif name == "no_shadow":
        use_shadow = False
    elif name == "compare":
        pcf = False
    elif name == "water_first":
        draws, surface = [wd] + objs, [True, False, False, False]
    elif name == "water_absent":
        draws, surface = objs, [False, False, False]
    elif name == "two_waters":
        far = water_draw(view, proj, water_grid(2, -4.0, 0.0, -5.0, 2.0, WATER_Y + 0.3))
        draws, surface = objs + [wd, far], [False, False, False, True, True]
    elif name == "nan_water":
        # a NaN corner: every clip coordinate of it is NaN, the triangle's depths are NaN and lose every depth test -- a hole
        # in the water that shows the floor below
        draws = objs[:1] + [dataclasses.replace(wd, mesh=_nan_vertex(wd.mesh, 9))] + objs[1:]
    elif name == "nan_normal":
        # u.model scales the water's world x and z by 1e36 under the same mvp: hash12's products overflow, fract(inf) is NaN
        # and so is N, while world_pos and with it the reflection lookup stay finite
        big = np.eye(4, dtype=F)
        big[0, 0] = big[2, 2] = 1e36
        draws = objs[:1] + [dataclasses.replace(wd, model=big.reshape(16))] + objs[1:]
    elif name == "nan_atmosphere":
        # a NaN corner on the floor (that triangle draws nothing) and zero-length normals on the monkey (glm::normalize gives
        # NaN: N and the colour are NaN in every fragment of the draw)
        mk = objs[1].mesh
        monkey0 = R.SoupMesh(mk.positions, np.zeros_like(mk.normals), getattr(mk, "uvs", None))
        draws = [dataclasses.replace(objs[0], mesh=_nan_vertex(objs[0].mesh, 3)), wd, dataclasses.replace(objs[1], mesh=monkey0), objs[2]]
    elif name == "time_w1":
        t = time_with_t0(0.0)
    elif name == "time_w0":
        t = time_with_t0(0.5)
    elif name == "time_1e4":
        t = 1e4
    elif name == "reflection_1x1":
        refl = distinct_image(1, 1)
    frame = water_frame(view, lvp, GRAZING_POS, w, h, tile, use_shadow=use_shadow, pcf=pcf)
    water = shs_gpu.RtWater(rvp, t, flag)
    return types.SimpleNamespace(frame=frame, draws=draws, surface=surface, water=water, reflection=refl, light_vp=lvp, sm=sm, tile=tile)


@functools.lru_cache(maxsize=None)
def scene_ref(name, witness=0):
    """The restatement's planes of a scene (computed once, shared, never written to)."""
    s = scene(name)
    ref_sm = R.ref_shadow(s.sm, s.light_vp, s.draws, s.tile)
    out = ref_render_water(s.frame, s.draws, s.surface, s.water, ref_sm if s.frame.use_shadow else None, s.reflection, witness)
    out["shadow_map"] = ref_sm
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def surface_of(s, tri_id):
    """Per pixel: does it show a water fragment"""
    bounds = np.cumsum([0] + [d.mesh.positions.shape[0] for d in s.draws])
    who = np.searchsorted(bounds, tri_id // 2, side="right") - 1
    return (tri_id >= 0) & np.asarray(s.surface + [False])[np.clip(who, 0, len(s.surface))]


# ---- what fails without the feature, without a GPU ---------------------------------------------------------------------

def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in ("shs_rt_render_water", "shs_rt_keep_reflection", "shs_rt_set_reflection", "shs_rt_water_samples", "shs_rt_render",
                 "shs_rt_render_skybox_ibl"):
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1
    import shs_gpu
    for name in ("rt_render_water", "rt_keep_reflection", "rt_set_reflection", "rt_water_samples"):
        assert hasattr(shs_gpu.Context, name), name
    assert shs_gpu.RtWaterDraw().surface is False and shs_gpu.RtWater().time_sec == 0.0 and shs_gpu.RtWater().reflection is False


def test_ctypes_structs_have_the_headers_layout(tmp_path):
    """sizeof and every member's offset of shs_rt_water_draw and shs_rt_water against the ctypes mirror; the flag values; the
    existing structs keep their sizes."""
    from shs_gpu import _abi
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) {\n'
                   '    size_t v[] = {sizeof(shs_rt_water_draw), offsetof(shs_rt_water_draw, flags), sizeof(shs_rt_water), '
                   'offsetof(shs_rt_water, reflection_vp), offsetof(shs_rt_water, time_sec), offsetof(shs_rt_water, flags), '
                   'SHS_RT_WATER_SURFACE, SHS_RT_WATER_REFLECTION, sizeof(shs_rt_frame), sizeof(shs_rt_draw), sizeof(shs_rt_skybox_ibl_draw)};\n'
                   '    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]);\n    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D, Wc = _abi.RtWaterDrawC, _abi.RtWaterC
    want = [ctypes.sizeof(D), D.flags.offset, ctypes.sizeof(Wc), Wc.reflection_vp.offset, Wc.time_sec.offset, Wc.flags.offset,
            _abi.RT_WATER_SURFACE, _abi.RT_WATER_REFLECTION, ctypes.sizeof(_abi.RtFrameC), ctypes.sizeof(_abi.RtDrawC),
            ctypes.sizeof(_abi.RtSkyboxIblDrawC)]
    assert got == want == [4, 0, 72, 0, 64, 68, 1, 1, 192, 204, 16]
    assert water_lib().rwt_sizeof_water() == ctypes.sizeof(RefWater) and water_lib().rwt_sizeof_debug() == ctypes.sizeof(RefDebug)


# ---- the second restatement: float32 numpy ---------------------------------------------------------------------------

def _fract(x):
    return (x - np.floor(x)).astype(F)


def np_hash12(px, py):
    """:771-777"""
    qx, qy = _fract(px * F(123.34)), _fract(py * F(456.21))
    d = (qx * (qx + F(34.345)) + qy * (qy + F(34.345))).astype(F)
    qx, qy = (qx + d).astype(F), (qy + d).astype(F)
    return _fract(qx * qy)


def np_hash22(p):
    """:779-796"""
    p = F(p)
    x, y, z = _fract(p * F(0.1031)), _fract(p * F(0.1030)), _fract(p * F(0.0973))
    d = F(F(x * (y + F(19.19)) + y * (z + F(19.19))) + z * (x + F(19.19)))
    x, y, z = _fract(x + d), _fract(y + d), _fract(z + d)
    return _fract((x + y) * z), _fract((x + z) * y)


def np_noise2(px, py):
    """:798-814"""
    ix, iy = np.floor(px), np.floor(py)
    fx, fy = (px - ix).astype(F), (py - iy).astype(F)
    a, b = np_hash12(ix + F(0), iy + F(0)), np_hash12(ix + F(1), iy + F(0))
    c, d = np_hash12(ix + F(0), iy + F(1)), np_hash12(ix + F(1), iy + F(1))
    ux, uy = (fx * fx * (F(3) - F(2) * fx)).astype(F), (fy * fy * (F(3) - F(2) * fy)).astype(F)
    x1 = a + (b - a) * ux
    x2 = c + (d - c) * ux
    return (x1 + (x2 - x1) * uy).astype(F)


def np_fbm2(px, py):
    """:816-826"""
    f, a = np.zeros_like(px), F(0.5)
    for _ in range(4):
        f = (f + a * np_noise2(px, py)).astype(F)
        px, py = (px * F(2.02)).astype(F), (py * F(2.02)).astype(F)
        a = F(a * F(0.5))
    return f


def _normalize(x, y, z):
    inv = F(1) / np.sqrt(((x * x + y * y) + z * z).astype(F))
    return (x * inv).astype(F), (y * inv).astype(F), (z * inv).astype(F)


def np_sample_n(px, py):
    """sampleN :902-917"""
    e, s = F(0.18), F(1.2)
    hx = np_fbm2((px + e) * s, (py + F(0)) * s) - np_fbm2((px - e) * s, (py - F(0)) * s)
    hz = np_fbm2((px + F(0)) * s, (py + e) * s) - np_fbm2((px - F(0)) * s, (py - e) * s)
    return _normalize((-hx * F(2.4)).astype(F), np.ones_like(px), (-hz * F(2.4)).astype(F))


def np_water_normal_foam(world, t):
    """water_flow_normal_and_foam :862-930 -> (N [n, 3], foam [n])"""
    with np.errstate(all="ignore"):
        world = np.asarray(world, F).reshape(-1, 3)
        x, z = world[:, 0], world[:, 2]
        inv = F(1) / np.sqrt(F(F(0.15) * F(0.15) + F(1) * F(1)))
        fdx, fdy = F(F(0.15) * inv), F(F(1) * inv)
        ppx, ppy = -fdy, fdx
        uvx = (x * ppx + z * ppy).astype(F)
        uvy = ((x * fdx + z * fdy).astype(F) * F(2.8)).astype(F)
        time = F(F(t) * F(0.18))
        t0, t1 = _fract(time), _fract(F(time + F(0.5)))
        w = F(np.abs(F(t0 - F(0.5))) * F(2))
        j0, j1 = np_hash22(np.floor(time)), np_hash22(np.floor(F(time + F(0.5))))
        uv = []
        for j, tt in ((j0, t0), (j1, t1)):
            k = F(tt - F(0.5))
            uv.append((((uvx * F(0.055)).astype(F) + F(j[0] * F(2))).astype(F) + F(F(fdx * k) * F(6)),
                       ((uvy * F(0.055)).astype(F) + F(j[1] * F(2))).astype(F) + F(F(fdy * k) * F(6))))
        ax, ay, az = np_sample_n(uv[0][0].astype(F), uv[0][1].astype(F))
        bx, by, bz = np_sample_n(uv[1][0].astype(F), uv[1][1].astype(F))
        iw = F(F(1) - w)
        nx, ny, nz = _normalize((ax * iw + bx * w).astype(F), (ay * iw + by * w).astype(F), (az * iw + bz * w).astype(F))
        nx, ny, nz = _normalize((nx + F(fdx * F(0.15))).astype(F), (ny + F(0)).astype(F), (nz + F(fdy * F(0.15))).astype(F))
        curv = np.sqrt((nx * nx + nz * nz).astype(F))
        v = ((curv - F(0.55)) * F(1.6)).astype(F)
        foam = np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)
    return np.stack([nx, ny, nz], -1), foam


def _lround_away(x):
    """(int)std::lround: halves away from zero on both sides; NaN -> (int)LONG_MIN = 0"""
    x = np.asarray(x, F)
    t = np.trunc(np.nan_to_num(x))
    d = np.nan_to_num(x) - t
    return (t + np.where(d >= 0.5, 1, np.where(d <= -0.5, -1, 0))).astype(np.int64)


def _ternary01(v):
    return np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)


def np_sky(ray, L):
    """sky_color_simple(normalize(RAY), normalize(-L)) :157-170 -> [n, 3]"""
    rx, ry, rz = _normalize(*ray)
    sun = _normalize(*_normalize(F(-L[0]), F(-L[1]), F(-L[2])))
    t = _ternary01((ry * F(0.5) + F(0.5)).astype(F))
    hor, zen = (F(0.62), F(0.74), F(0.92)), (F(0.10), F(0.22), F(0.55))
    nx, ny, nz = _normalize(rx, ry, rz)
    sd = ((sun[0] * nx + sun[1] * ny).astype(F) + sun[2] * nz).astype(F)
    s = np.power(_ternary01((sd * F(0.5) + F(0.5)).astype(F)), F(256)).astype(F)
    glow = (F(1.0), F(0.88), F(0.65))
    return [((hor[k] * (F(1) - t) + zen[k] * t).astype(F) + ((glow[k] * s).astype(F) * F(8)).astype(F)).astype(F) for k in range(3)]


def np_water_shadow(frame, shadow_map, ndl, world):
    """shadow_uvz_from_world :696-714, the bias, shadow_factor_pcf_2x2 :716-751 -> [n]"""
    n = len(ndl)
    out = np.ones(n, F)
    if not frame.use_shadow:
        return out
    sm = np.asarray(shadow_map, F)
    sh, sw = sm.shape
    cx, cy, cz, cw = I._m4v(frame.light_vp, np.asarray(world, F))
    with np.errstate(all="ignore"):
        nx, ny, z = (cx / cw).astype(F), (cy / cw).astype(F), (cz / cw).astype(F)
        called = ~(np.abs(cw) < F(1e-6)) & ~((z < 0) | (z > 1))
        u = (nx * F(0.5) + F(0.5)).astype(F)
        v = (F(1) - (ny * F(0.5) + F(0.5))).astype(F)
        inside = ~((u < 0) | (u > 1) | (v < 0) | (v > 1))
        slope = F(1) - K._clamp(ndl, 0, 1)
        bias = (F(frame.bias_base) + F(frame.bias_slope) * slope).astype(F)
        fx, fy = (u * F(sw - 1)).astype(F), (v * F(sh - 1)).astype(F)

        def lit(x, y):
            d = sm[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)]
            return np.where(d == helpers.FLT_MAX, F(1), np.where(z <= (d + bias).astype(F), F(1), F(0))).astype(F)
        if frame.pcf:
            x0 = np.clip(np.floor(np.nan_to_num(fx)).astype(np.int64), 0, sw - 1)
            y0 = np.clip(np.floor(np.nan_to_num(fy)).astype(np.int64), 0, sh - 1)
            x1, y1 = np.clip(x0 + 1, 0, sw - 1), np.clip(y0 + 1, 0, sh - 1)
            s = (F(0.25) * (((lit(x0, y0) + lit(x1, y0)) + lit(x0, y1)) + lit(x1, y1))).astype(F)
        else:
            s = lit(_lround_away(fx), _lround_away(fy))
    return np.where(called & inside, s, out).astype(F)


def np_fragments(frame, water, surface, normal, world, base, shadow_map=None, reflection=None):
    """Both shaders in float32 numpy -> (pre [n, 4], N [n, 3], foam [n])"""
    with np.errstate(all="ignore"):
        world = np.asarray(world, F).reshape(-1, 3)
        n = world.shape[0]
        surface = np.broadcast_to(np.asarray(surface, bool), (n,))
        ld = [F(v) for v in frame.light_dir_world]
        L = _normalize(-ld[0], -ld[1], -ld[2])
        cam = [F(v) for v in frame.camera_pos]
        tc = [(cam[k] - world[:, k]).astype(F) for k in range(3)]
        V = _normalize(*tc)
        sky = np_sky((-V[0], -V[1], -V[2]), L)
        wN, foam = np_water_normal_foam(world, water.time_sec)
        nn = np.asarray(normal, F).reshape(-1, 3)
        aN = np.stack(_normalize(nn[:, 0], nn[:, 1], nn[:, 2]), -1)
        N = np.where(surface[:, None], wN, aN).astype(F)
        foam = np.where(surface, foam, F(0)).astype(F)

        def dot(a, b):
            return ((a[0] * b[0] + a[1] * b[1]).astype(F) + a[2] * b[2]).astype(F)
        Nc = (N[:, 0], N[:, 1], N[:, 2])
        ndl, ndv = dot(Nc, L), dot(Nc, V)
        shadow = np_water_shadow(frame, shadow_map, ndl, world)
        Hh = _normalize((L[0] + V[0]).astype(F), (L[1] + V[1]).astype(F), (L[2] + V[2]).astype(F))
        ndh = np.where(dot(Nc, Hh) < 0, F(0), dot(Nc, Hh)).astype(F)
        # the water shader
        NoV, NoL = K._clamp(ndv, 0, 1), K._clamp(ndl, 0, 1)
        fres = (F(0.02) + F(F(1) - F(0.02)) * np.power((F(1) - NoV).astype(F), F(5)).astype(F)).astype(F)
        refl = [s.copy() for s in sky]
        if water.reflection:
            img = np.asarray(reflection, np.uint8)
            rh, rw = img.shape[:2]
            cx, cy, cz, cw = I._m4v(np.asarray(water.reflection_vp, F).reshape(16), world)
            ok = np.abs(cw) > F(1e-6)
            rx_, ry_ = (cx / cw).astype(F), (cy / cw).astype(F)
            ok &= (rx_ >= -1) & (rx_ <= 1) & (ry_ >= -1) & (ry_ <= 1)
            sx = ((rx_ * F(0.5) + F(0.5)).astype(F) * F(rw - 1)).astype(F)
            sy = ((F(1) - (ry_ * F(0.5) + F(0.5))).astype(F) * F(rh - 1)).astype(F)
            sx, sy = (sx + (N[:, 0] * F(0.75)).astype(F)).astype(F), (sy + (N[:, 2] * F(0.75)).astype(F)).astype(F)
            rx, ryc = _lround_away(sx), (rh - 1) - _lround_away(sy)
            tex = img[np.clip(ryc, 0, rh - 1), np.clip(rx, 0, rw - 1)]
            for k in range(3):
                refl[k] = np.where(ok, (tex[:, k].astype(F) / F(255)).astype(F), refl[k]).astype(F)
        spec = np.power(ndh, F(520)).astype(F)
        specular = (((F(1) * spec) * F(0.95)).astype(F) * (F(1) - foam * F(0.90)).astype(F)).astype(F)
        diffuse = ((F(1) * NoL) * F(0.05)).astype(F)
        fgain = (foam * (F(0.35) + F(0.65) * (F(1) - NoV)).astype(F)).astype(F)
        wb, fb = (F(0.03), F(0.12), F(0.16)), (F(0.75), F(0.85), F(0.95))
        sd, ss = (shadow * diffuse).astype(F), (shadow * specular).astype(F)
        # the atmosphere shader
        b = np.asarray(base, np.uint8).reshape(n, 3).astype(F) / F(255)
        adiff = ((F(1) * np.where(ndl < 0, F(0), ndl)) * F(0.90)).astype(F)
        aspec = ((F(1) * np.power(ndh, F(64)).astype(F)) * F(0.35)).astype(F)
        alit = (shadow * (adiff + aspec).astype(F)).astype(F)
        dist = np.sqrt(dot(tc, tc))
        dist = np.where(dist < 0, F(0), np.where(dist > 250, F(250), dist)).astype(F)
        tr = np.exp2((F(-0.0065) * dist).astype(F)).astype(F)
        pre = np.empty((n, 4), F)
        for k in range(3):
            surf = (wb[k] * (F(1) - fres) + refl[k] * fres).astype(F)
            fcol = (fb[k] * F(0.75) + sky[k] * F(0.25)).astype(F)
            surf = (surf * (F(1) - fgain) + fcol * fgain).astype(F)
            hw = ((surf * ((sky[k] * F(0.12)).astype(F) + sd).astype(F)).astype(F) + ss).astype(F)
            ha = (b[:, k] * ((sky[k] * F(0.08)).astype(F) + alit).astype(F)).astype(F)
            hdr = np.where(surface, hw, ha).astype(F)
            hdr = ((hdr * tr).astype(F) + (sky[k] * (F(1) - tr)).astype(F)).astype(F)
            hdr = (hdr * np.where(surface, F(0.90), F(1.0)).astype(F)).astype(F)
            c = K._clamp((hdr / (F(1) + hdr)).astype(F), 0, 1)
            pre[:, k] = (np.power(c, F(1.0) / F(2.2)).astype(F) * F(255)).astype(F)
        pre[:, 3] = shadow
    return pre, N, foam


def seeded_points(seed=11, n=600):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-30, 30, (n, 3)), rng.uniform(-1e3, 1e3, (n // 2, 3)), rng.uniform(-1e6, 1e6, (n // 2, 3)),
                          [[0, 0, 0], [-0.0, 0.0, -0.0], [1e6, 0, -1e6], [-1e6, 0, 1e6], [np.nan, 0, 0], [0, 0, np.nan], [np.inf, 0, 1],
                           [1, 0, -np.inf], [np.inf, 0, np.inf]]]).astype(F)
    return pts


SAMPLE_TIMES = (0.0, 3.7, 1e4)


def sample_times():
    return SAMPLE_TIMES + (time_with_t0(0.0), time_with_t0(0.5))


def test_times_with_exact_blend_weights_exist():
    for want, w in ((0.0, 1.0), (0.5, 0.0)):
        t = time_with_t0(want)
        time = F(t) * F(0.18)
        t0 = time - np.floor(time)
        assert t > 0 and t0 == F(want) and abs(t0 - F(0.5)) * F(2) == F(w)


def test_normal_and_foam_equal_the_numpy_restatement_bitwise():
    pts = seeded_points()
    for t in sample_times():
        cn, cf = ref_water_samples(pts, t)
        nn, nf = np_water_normal_foam(pts, t)
        bad = np.argwhere((P.canonical_bits(cn) != P.canonical_bits(nn)).any(-1) | (P.canonical_bits(cf) != P.canonical_bits(nf)))
        assert bad.size == 0, f"t = {t}: {len(bad)} of {len(pts)} points differ, first {pts[bad[:3, 0]].tolist()}"
        fin = np.isfinite(pts).all(-1)
        assert np.isfinite(cn[fin]).all() and np.isnan(cn[~fin]).any(-1).all()
        assert np.abs(np.linalg.norm(cn[fin].astype(np.float64), axis=-1) - 1).max() < 1e-6 and (cf[fin] >= 0).all() and (cf[fin] <= 1).all()
        assert np.isnan(cf[~fin]).all()
    # the points differ among themselves and over time: the chain is not degenerate
    a, b = ref_water_samples(pts, 3.7)[0], ref_water_samples(pts, 1e4)[0]
    assert len(np.unique(a[np.isfinite(a).all(-1)], axis=0)) > 1000 and (np.abs(a - b) > 1e-3).any(-1).mean() > 0.9


def test_hash12_known_answers():
    """hash12 at lattice points by hand-ordered float32 operations (:771-777), and the chain above it at a lattice point:
    noise2 of a lattice point is hash12 of it, fbm2 sums four of them."""
    L = water_lib()
    for x, y in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (3.0, -2.0), (-7.0, 11.0), (101.0, 57.0)):
        a, b = F(x) * F(123.34), F(y) * F(456.21)
        qx, qy = F(a - np.floor(a)), F(b - np.floor(b))
        d = F(F(qx * F(qx + F(34.345))) + F(qy * F(qy + F(34.345))))
        qx, qy = F(qx + d), F(qy + d)
        p = F(qx * qy)
        want = F(p - np.floor(p))
        got = F(L.rwt_hash12(x, y))
        assert got == want and 0 <= got < 1, (x, y, got, want)
        assert F(L.rwt_noise2(x, y)) == want       # f = 0: u = 0, x1 = a, the result a
    assert L.rwt_hash12(0.0, 0.0) == 0.0
    h = (ctypes.c_float * 2)()
    L.rwt_hash22(3.0, h)
    assert (F(h[0]), F(h[1])) == tuple(F(v) for v in np_hash22(3.0)) and 0 <= h[0] < 1 and 0 <= h[1] < 1
    p = F(F(5.0) * F(0.1031))
    p = F(p - np.floor(p))
    p = F(p * F(p + F(33.33)))
    p = F(p * F(p + p))
    assert F(L.rwt_hash11(5.0)) == F(p - np.floor(p))


def test_foam_and_fresnel_known_answers():
    import shs_gpu
    view, _ = look(GRAZING_POS, GRAZING_TARGET)
    water = shs_gpu.RtWater(None, 0.0, False)
    # foam is clamp01((length(N.xz) - 0.55) * 1.6): zero for a normal within 0.55 of the vertical -- the flat normal plus the
    # flow tilt, (0.15 fd.x, 1, 0.15 fd.y) normalised, has length(N.xz) = 0.148
    fd = np.array([0.15, 1.0]) / np.hypot(0.15, 1.0)
    flat = np.array([0.15 * fd[0], 1.0, 0.15 * fd[1]])
    flat /= np.linalg.norm(flat)
    assert np.hypot(flat[0], flat[2]) < 0.55
    pts = seeded_points()[:600]
    n, foam = ref_water_samples(pts, 3.7)
    curv = np.hypot(n[:, 0].astype(np.float64), n[:, 2].astype(np.float64))
    assert (foam[curv < 0.549] == 0).all() and (foam[curv > 0.551] > 0).all() and (curv < 0.549).any() and (curv > 0.551).any()
    # fresnel: the camera straight above a point whose normal is N sees NoV = N.y; at grazing NoV -> 0 and fresnel -> 1
    for cam, overhead in (((0.0, 1e4, 0.0), True), ((1e4, WATER_Y + 1e-3, 0.0), False)):
        frame = water_frame(view, R.light(), cam, use_shadow=False)
        pre, _, d = ref_fragments(frame, water, 1, np.zeros((50, 3)), np.c_[pts[:50, 0], np.full(50, WATER_Y), pts[:50, 2]], np.zeros((50, 3), np.uint8))
        N = d["normal"].astype(np.float64)
        V = np.asarray(cam) - np.c_[pts[:50, 0], np.full(50, WATER_Y), pts[:50, 2]].astype(np.float64)
        V /= np.linalg.norm(V, axis=-1, keepdims=True)
        nov = np.clip((N * V).sum(-1), 0, 1)
        assert np.abs(d["fresnel"] - (0.02 + 0.98 * (1 - nov) ** 5)).max() < 1e-5
        assert (d["fresnel"] >= F(0.02)).all() and (d["fresnel"] <= 1).all() and (d["branch"] == REFL_NONE).all()
        if overhead:
            assert (d["fresnel"] < 0.2).all()
        else:
            assert np.median(d["fresnel"]) > 0.5 and d["fresnel"].max() > 0.99
    # exactly F0 where N.V = 1 cannot be arranged through the noise; the formula's end points are the restatement's own
    assert F(0.02) + F(F(1) - F(0.02)) * F(0) == F(0.02)


def test_reflection_texel_known_answers():
    """A reflection canvas of distinct texels names the texel: the colour of a water fragment with fresnel near 1 is the
    texel (rx, ry_canvas) of the debug output, which is lround(sx + 0.75 N.x), (h - 1) - lround(sy + 0.75 N.z) over the
    reflection's own size, clamped; lround rounds negative halves away from zero."""
    import shs_gpu
    L = water_lib()
    for x, want in ((-0.75, -1), (-0.5, -1), (-0.49999997, 0), (-0.25, 0), (0.5, 1), (1.5, 2), (2.4999998, 2), (95.5, 96), (95.75, 96),
                    (float("nan"), 0)):
        assert L.rwt_lround(x) == want and int(_lround_away(F(x))) == want, x
    img = distinct_image(72, 48)
    rw, rh = 72, 48
    # an orthographic reflection_vp over the water's x, z: rndc = (x / 14, (z - 11.5) / 18.5)
    rvp = np.zeros((4, 4), F)
    rvp[0, 0], rvp[2, 1], rvp[3, 1], rvp[3, 3] = 1 / 14.0, 1 / 18.5, -11.5 / 18.5, 1.0
    water = shs_gpu.RtWater(rvp.reshape(16), 3.7, True)
    view, _ = look(GRAZING_POS, GRAZING_TARGET)
    frame = water_frame(view, R.light(), (1e4, WATER_Y + 1e-3, 0.0), use_shadow=False)
    rng = np.random.default_rng(3)
    pts = np.c_[rng.uniform(-14, 14, 400), np.full(400, WATER_Y), rng.uniform(-7, 30, 400)].astype(F)
    pts[:4] = [[-14, WATER_Y, -7], [14, WATER_Y, 30], [-14, WATER_Y, 30], [14, WATER_Y, -7]]        # the corners: sx, sy at both ends
    pre, rgba, d = ref_fragments(frame, water, 1, np.zeros((400, 3)), pts, np.zeros((400, 3), np.uint8), reflection=img)
    assert (d["branch"] == REFL_TEXEL).all()
    N = d["normal"]
    sx = ((pts[:, 0] / F(14.0) * F(0.5) + F(0.5)) * F(rw - 1)).astype(np.float64) + 0.75 * N[:, 0]
    sy = ((1 - ((pts[:, 2] - 11.5) / 18.5 * 0.5 + 0.5)) * (rh - 1)).astype(np.float64) + 0.75 * N[:, 2]
    near_half = (np.abs(sx - np.floor(sx) - 0.5) < 1e-3) | (np.abs(sy - np.floor(sy) - 0.5) < 1e-3)
    rx, ry = np.floor(sx + 0.5).astype(int), (rh - 1) - np.floor(sy + 0.5).astype(int)
    ok = ~near_half
    assert ok.sum() > 350 and (d["rx"][ok] == rx[ok]).all() and (d["ry_canvas"][ok] == ry[ok]).all()
    assert sorted(zip(d["rx"][:4].tolist(), d["ry_canvas"][:4].tolist())) == [(0, 0), (0, rh - 1), (rw - 1, 0), (rw - 1, rh - 1)]
    # the numpy restatement reads the same texel, and the colour follows it: another texel is another colour
    pre2, _, _ = np_fragments(frame, water, True, np.zeros((400, 3)), pts, np.zeros((400, 3), np.uint8), reflection=img)
    assert np.abs(pre2[:, :3] - pre[:, :3]).max() <= BAR
    shifted = np.roll(img, 1, axis=1)
    pre3, _, _ = ref_fragments(frame, water, 1, np.zeros((400, 3)), pts, np.zeros((400, 3), np.uint8), reflection=shifted)
    assert (np.abs(pre3[:, :3] - pre[:, :3]).max(-1) > 100 * BAR).mean() > 0.9
    # a NaN normal under a finite lookup: at x = 3e37 hash12's product overflows, fract(inf) is NaN and so is N, while
    # reflection_vp (scaled down) keeps rndc finite and inside; sx and sy are NaN, lround gives (int)LONG_MIN = 0:
    # rx = 0, ry_canvas = h - 1.  (A NaN position never gets here: rclip.w is NaN and the |w| test is false.)
    small = np.eye(4, dtype=F)
    small[0, 0] = 1e-38
    wnan = shs_gpu.RtWater(small.reshape(16), 3.7, True)
    _, _, d = ref_fragments(frame, wnan, 1, np.zeros((2, 3)), [[3e37, -0.5, 1.0], [np.nan, -0.5, 1.0]], np.zeros((2, 3), np.uint8), reflection=img)
    assert d["branch"][0] == REFL_TEXEL and np.isnan(d["normal"][0]).all() and (d["rx"][0], d["ry_canvas"][0]) == (0, rh - 1)
    assert d["branch"][1] == REFL_W and np.isnan(d["normal"][1]).all()


def test_shadow_factor_known_answers():
    """Outside the light's uv square the water demo's lookup is lit before the taps; the hard demo's PCF clamps the taps to
    the edge and compares.  One fragment where they differ; and an empty texel under a NaN z."""
    L, HL = water_lib(), R.ref_lib()
    sm = np.full((8, 8), 0.2, F)
    ptr = sm.ctypes.data
    for pcf in (0, 1):
        assert L.rwt_shadow_factor(ptr, 8, 8, pcf, 1.2, 0.5, 0.6, 0.0) == 1.0
        assert L.rwt_shadow_factor(ptr, 8, 8, pcf, 0.5, -0.01, 0.6, 0.0) == 1.0
        assert L.rwt_shadow_factor(ptr, 8, 8, pcf, 0.5, 0.5, 0.6, 0.0) == 0.0
        assert L.rwt_shadow_factor(ptr, 8, 8, pcf, 0.5, 0.5, 0.1, 0.0) == 1.0
    assert HL.rcr_shadow_pcf(ptr, 8, 8, 1.2, 0.5, 0.6, 0.0) == 0.0          # the hard demo: the edge texels shadow it
    assert HL.rcr_shadow_compare(ptr, 8, 8, 1.2, 0.5, 0.6, 0.0) == 1.0       # (its compare path has the range test)
    sm[3, 4] = 0.9
    assert L.rwt_shadow_factor(ptr, 8, 8, 1, 3.5 / 7, 2.5 / 7, 0.6, 0.0) == 0.25
    empty = np.full((8, 8), helpers.FLT_MAX, F)
    assert L.rwt_shadow_factor(empty.ctypes.data, 8, 8, 1, 0.5, 0.5, float("nan"), 0.0) == 1.0
    assert HL.rcr_shadow_pcf(empty.ctypes.data, 8, 8, 0.5, 0.5, float("nan"), 0.0) == 0.0


def _random_fragments(seed, n=400):
    rng = np.random.default_rng(seed)
    world = np.c_[rng.uniform(-14, 14, n), rng.uniform(-0.5, 3.0, n), rng.uniform(-7, 30, n)].astype(F)
    normal = rng.normal(size=(n, 3)).astype(F)
    normal[:5] = 0
    base = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    surface = rng.random(n) < 0.5
    world[-3:] = [[np.nan, 0, 0], [0, np.inf, 0], [1, 2, np.nan]]
    return world, normal, base, surface


@pytest.mark.parametrize("use_shadow,pcf", [(True, True), (True, False), (False, True)], ids=["pcf", "compare", "no-map"])
@pytest.mark.parametrize("refl", ["distinct", "none"])
def test_fragments_equal_the_numpy_restatement(use_shadow, pcf, refl):
    import shs_gpu
    s = scene("host_reflection")
    ref_sm = scene_ref("host_reflection")["shadow_map"]
    frame = dataclasses.replace(s.frame, use_shadow=use_shadow, pcf=pcf)
    water = dataclasses.replace(s.water, reflection=refl == "distinct")
    img = s.reflection if refl == "distinct" else None
    world, normal, base, surface = _random_fragments(21)
    for t in (3.7, time_with_t0(0.5)):
        wt = dataclasses.replace(water, time_sec=t)
        pre, rgba, d = ref_fragments(frame, wt, surface.astype(np.int32), normal, world, base, ref_sm, img)
        npre, nN, nfoam = np_fragments(frame, wt, surface, normal, world, base, ref_sm, img)
        assert np.array_equal(P.canonical_bits(d["normal"]), P.canonical_bits(nN)) and np.array_equal(P.canonical_bits(d["foam"]), P.canonical_bits(nfoam))
        assert np.array_equal(P.canonical_bits(pre[:, 3]), P.canonical_bits(npre[:, 3])), "shadow factors"
        assert np.array_equal(np.isnan(pre), np.isnan(npre))
        with np.errstate(invalid="ignore"):
            assert np.nanmax(np.abs(pre[:, :3] - npre[:, :3])) <= BAR
        fin = ~np.isnan(pre[:, :3]).any(-1)
        assert (rgba[fin][:, :3] == np.clip(np.floor(pre[fin][:, :3].astype(np.float64) + 0.5), 0, 255)).all(), "the bytes round"
        assert (rgba[~fin][:, :3][np.isnan(pre[~fin][:, :3])] == 0).all() and (rgba[:, 3] == 255).all()
        if use_shadow:
            assert len(np.unique(pre[fin][:, 3])) >= (3 if pcf else 2)
        assert (d["branch"][~surface] == ATMOSPHERE).all() and set(np.unique(d["branch"][surface])) <= ({REFL_TEXEL, REFL_OUTSIDE, REFL_W} if img is not None else {REFL_NONE})
        assert not ((d["branch"] == REFL_W) & np.isfinite(world).all(-1)).any()      # (|NaN| > 1e-6 is false)


def test_raster_planes_equal_shading_0s_restatement():
    """ids, depth and velocity of the same draws under shading 0's restatement and this one are bit-identical, and so are the
    counters: the raster is the hard demo's."""
    for name in ("host_reflection", "two_waters", "nan_water", "uneven_tile"):
        s, ref = scene(name), scene_ref(name)
        hard = R.ref_render(dataclasses.replace(s.frame, shading=0), s.draws, ref["shadow_map"] if s.frame.use_shadow else None)
        for k in ("tri_id", "depth", "velocity"):
            assert np.array_equal(P.canonical_bits(hard[k]) if hard[k].dtype == F else hard[k], P.canonical_bits(ref[k]) if ref[k].dtype == F else ref[k]), (name, k)
        assert hard["counters"] == ref["counters"]
        assert (hard["prequant"][..., :3] != ref["prequant"][..., :3]).any()


def test_scenes_show_their_edges():
    """Each edge the GPU test names occurs in its scene, by the restatement's debug planes."""
    def water_px(name):
        s, ref = scene(name), scene_ref(name)
        return s, ref, surface_of(s, ref["tri_id"])
    s, ref, wpx = water_px("host_reflection")
    assert wpx.sum() > 5000 and (ref["tri_id"] >= 0).sum() - wpx.sum() > 2000 and (ref["tri_id"] < 0).sum() > 500
    assert (ref["branch"][wpx] == REFL_TEXEL).mean() > 0.9 and (ref["branch"][~wpx & (ref["tri_id"] >= 0)] == ATMOSPHERE).all()
    assert s.reflection.shape[:2] != (s.frame.height, s.frame.width)
    rxy = ref["rxy"][wpx & (ref["branch"] == REFL_TEXEL)]
    assert np.ptp(rxy[:, 0]) > 60 and np.ptp(rxy[:, 1]) > 15
    assert (ref["fresnel"][wpx] > 0.3).mean() > 0.5, "a grazing camera: fresnel is large"
    # uv leaves [0, 1] inside the frame, on water pixels, and the factor there is 1; inside it all five PCF values occur
    out = (ref["flags"] & R.PX_SUV_OUTSIDE) != 0
    assert (out & wpx).sum() > 500 and (ref["prequant"][out][:, 3] == 1).all() and len(np.unique(ref["prequant"][wpx & ~out][:, 3])) >= 4
    hard = R.ref_render(dataclasses.replace(s.frame, shading=0), s.draws, ref["shadow_map"])
    assert (hard["prequant"][out & wpx][:, 3] != 1).any(), "the hard demo's PCF gives another factor on some of them"
    _, ref, wpx = water_px("no_reflection")
    assert (ref["branch"][wpx] == REFL_NONE).all()
    _, ref, wpx = water_px("outside")
    b = ref["branch"][wpx]
    assert (b == REFL_OUTSIDE).sum() > 1000 and (b == REFL_TEXEL).sum() > 1000
    s = scene("outside")
    _, _, d = ref_fragments(dataclasses.replace(s.frame, use_shadow=False), s.water, 1, np.zeros((1, 3)), [[0.0, WATER_Y, -5.0]],
                            np.zeros((1, 3), np.uint8), reflection=s.reflection)
    cw = I._m4v(s.water.reflection_vp, np.array([[0.0, WATER_Y, -5.0]], F))[3]
    assert cw[0] < -1 and d["branch"][0] in (REFL_TEXEL, REFL_OUTSIDE), "behind the mirrored camera the |w| test passes"
    _, ref, wpx = water_px("w_tiny")
    b = ref["branch"][wpx]
    assert (b == REFL_W).sum() > 1000 and (b == REFL_OUTSIDE).sum() > 100 and (b == REFL_TEXEL).sum() == 0
    _, ref, wpx = water_px("no_shadow")
    assert (ref["prequant"][ref["tri_id"] >= 0][:, 3] == 1).all()
    _, ref, wpx = water_px("compare")
    assert set(np.unique(ref["prequant"][wpx][:, 3])) == {0.0, 1.0}
    _, ref, wpx = water_px("water_absent")
    assert wpx.sum() == 0 and (ref["tri_id"] >= 0).sum() > 3000
    s, ref, wpx = water_px("two_waters")
    who = np.searchsorted(np.cumsum([0] + [d.mesh.positions.shape[0] for d in s.draws]), ref["tri_id"] // 2, side="right") - 1
    assert ((who == 3) & wpx).sum() > 1000 and ((who == 4) & wpx).sum() > 100
    a, b = scene_ref("water_first"), scene_ref("host_reflection")
    assert np.array_equal(a["color"], b["color"]) and not np.array_equal(a["tri_id"], b["tri_id"])
    s, ref, wpx = water_px("nan_water")
    hole = ~wpx & surface_of(scene("host_reflection"), scene_ref("host_reflection")["tri_id"])
    assert hole.sum() > 20 and not np.isnan(ref["prequant"]).any()
    s, ref, wpx = water_px("nan_normal")
    tex = wpx & (ref["branch"] == REFL_TEXEL)
    assert wpx.sum() > 5000 and np.isnan(ref["normal"][wpx]).all() and tex.sum() > 3000
    assert (ref["rxy"][tex] == (0, s.reflection.shape[0] - 1)).all()
    assert np.isnan(ref["prequant"][wpx][:, :3]).all() and (ref["color"][wpx][:, :3] == 0).all()
    s, ref, wpx = water_px("nan_atmosphere")
    assert (np.isnan(ref["prequant"][..., :3]).any(-1) & ~wpx & (ref["tri_id"] >= 0)).sum() > 20
    # w = 1 at time = 1 shows sample B alone (cell floor(1.5) = 1, offset 0) and w = 0 at time = 1.5 sample A alone (cell
    # floor(1.5) = 1, offset 0): the same normals, which are not those of another time
    assert (time_with_t0(0.0), time_with_t0(0.5)) == (float(F(1 / 0.18)), float(F(1.5 / 0.18)))
    assert np.array_equal(scene_ref("time_w0")["normal"], scene_ref("time_w1")["normal"])
    assert not np.array_equal(scene_ref("time_w0")["normal"], scene_ref("host_reflection")["normal"])
    s, ref, wpx = water_px("reflection_1x1")
    assert (ref["branch"][wpx] == REFL_TEXEL).mean() > 0.9 and wpx.sum() > 5000      # (w - 1 = h - 1 = 0: every lookup is the one texel)
    s, ref, wpx = water_px("one_pixel_high")
    # (H - 1 = 0 scales every screen y to 0: no sub-triangle has an area, the frame is the clear colour)
    assert ref["tri_id"].shape == (1, 160) and ref["counters"]["sub_tris"] == 0 and (ref["tri_id"] == -1).all()
    for name in SCENE_NAMES:
        assert scene(name).frame.clear_color == CLEAR_BG


HASH_SHARE = TEXEL_SHARE = 0.5


@pytest.mark.parametrize("name", SCENE_NAMES + ("demo",))
def test_witnesses(name):
    """So that the GPU comparison cannot hide a wrong normal or a wrong texel: per scene the GPU test compares, one ulp on
    hash12's first input moves a colour float by more than 100 bars on at least half the water pixels (whose colour is
    not NaN), and in the scenes whose reflection has distinct texels a lookup one texel to the right does so on at least
    half the water pixels that read a texel."""
    if name == "demo":
        s, ref, hashed, shifted = demo_frame_ref(), None, None, None
        ref, hashed = s["main"], s["main_hash_witness"]
        wpx = s["water_px"]
    else:
        sc = scene(name)
        ref, hashed = scene_ref(name), scene_ref(name, WITNESS_HASH_ULP)
        wpx = surface_of(sc, ref["tri_id"])
        shifted = scene_ref(name, WITNESS_SHIFT_TEXEL) if sc.reflection is not None and sc.reflection.shape[0] > 1 else None
    if wpx.sum() == 0:
        assert name in ("water_absent", "one_pixel_high")
        return
    with np.errstate(invalid="ignore"):
        fin = wpx & ~np.isnan(ref["prequant"][..., :3]).any(-1)
        if name == "nan_normal":
            assert fin.sum() == 0           # (every water pixel's colour is NaN: there is nothing a witness could move)
            return
        moved = np.abs(hashed["prequant"][..., :3] - ref["prequant"][..., :3]).max(-1) > 100 * BAR
        share = moved[fin].mean()
        print(f"{name}: one ulp on a hash12 input moves {share:.3f} of {fin.sum()} water pixels by more than 100 bars")
        assert share >= HASH_SHARE
        for k in ("tri_id", "depth", "velocity"):
            assert np.array_equal(hashed[k], ref[k], equal_nan=True)
        if shifted is not None:
            tex = fin & (ref["branch"] == REFL_TEXEL)
            if tex.sum():
                moved = np.abs(shifted["prequant"][..., :3] - ref["prequant"][..., :3]).max(-1) > 100 * BAR
                share = moved[tex].mean()
                print(f"{name}: a lookup one texel off moves {share:.3f} of {tex.sum()} texel-reading water pixels by more than 100 bars")
                assert share >= TEXEL_SHARE


# ---- the demo's frame in order (shared with the GPU test) ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def demo_frame():
    """hello_water.cpp's frame at 160 x 120: the reflection pass from the mirrored camera (every draw non-water, no reflection
    bound, the mirrored position as camera_pos :1804) and the camera pass with floor, water and objects."""
    import shs_gpu
    view, proj = look(GRAZING_POS, GRAZING_TARGET)
    rview, rproj, rpos = mirrored(GRAZING_POS, GRAZING_TARGET)
    lvp = R.light()
    t = 12.5
    objs = objects(view, proj)
    main_draws = objs[:1] + [water_draw(view, proj)] + objs[1:]
    return types.SimpleNamespace(
        view=view, proj=proj, light_vp=lvp, sm=SM, tile=(80, 80),
        refl_frame=water_frame(rview, lvp, rpos), refl_draws=objects(rview, rproj), refl_surface=[False] * 3,
        refl_water=shs_gpu.RtWater(None, t, False),
        main_frame=water_frame(view, lvp, GRAZING_POS), main_draws=main_draws, main_surface=[False, True, False, False],
        main_water=shs_gpu.RtWater(R._mul(rproj, rview), t, True))


@functools.lru_cache(maxsize=None)
def demo_frame_ref():
    d = demo_frame()
    sm = R.ref_shadow(d.sm, d.light_vp, d.main_draws, d.tile)
    refl = ref_render_water(d.refl_frame, d.refl_draws, d.refl_surface, d.refl_water, sm)
    main = ref_render_water(d.main_frame, d.main_draws, d.main_surface, d.main_water, sm, refl["color"])
    hashed = ref_render_water(d.main_frame, d.main_draws, d.main_surface, d.main_water, sm, refl["color"], WITNESS_HASH_ULP)
    wpx = surface_of(types.SimpleNamespace(draws=d.main_draws, surface=d.main_surface), main["tri_id"])
    return {"shadow_map": sm, "reflection": refl, "main": main, "main_hash_witness": hashed, "water_px": wpx}


def test_the_demos_frame_reflects_the_scene():
    r = demo_frame_ref()
    refl, main, wpx = r["reflection"], r["main"], r["water_px"]
    assert (refl["tri_id"] >= 0).sum() > 2000 and (refl["branch"][refl["tri_id"] >= 0] == ATMOSPHERE).all()
    assert wpx.sum() > 5000 and (main["branch"][wpx] == REFL_TEXEL).mean() > 0.9
    # the water shows the reflection pass's colours: with the clear colour in place of the canvas the frame differs
    d = demo_frame()
    flat = np.empty_like(refl["color"])
    flat[:] = CLEAR_BG
    other = ref_render_water(d.main_frame, d.main_draws, d.main_surface, d.main_water, r["shadow_map"], flat)
    assert (np.abs(other["prequant"][..., :3] - main["prequant"][..., :3]).max(-1)[wpx] > 100 * BAR).mean() > 0.1
