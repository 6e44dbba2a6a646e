"""tests/canvas_rt_skybox_ibl_ref (ref_canvas_rt_skybox_ibl.c), the C restatement of hello_ibl_skybox.cpp's camera pass --
the hard demo's raster with the sky-lit fragment_shader_full (:446-524) -- the reference of
tests/test_canvas_rt_skybox_ibl.py, pinned on the CPU:

  * against a second restatement of the shader in float32 numpy, written from the same cited lines, on seeded random
    fragments (normals of any length, zero and NaN ones, the cube's axes and face diagonals; knobs below 0, inside (0, 1)
    and above 1) under no sky, the analytic sky and a cubemap sky, with and without the shadow map and the PCF;
  * against shading 0's restatement: with a white base colour, no texture and either no sky or ibl_ambient = ibl_refl = 0
    the two shaders perform the same operations, so every plane is equal bit for bit; with another base colour the
    frames differ where the specular term is not zero (it does not take the base colour here);
  * by known answers: F = ibl_f0 facing the camera and F -> 1 at grazing incidence; under a cubemap of six flat colours
    the tint and the reflection name the face N and R point into;
  * with the ABI struct's size and offsets against the ctypes mirror.

It also holds the wrapper, the knob sets and the frames the GPU test shares, and what fails without the feature and
needs no GPU: the new entry point and the struct."""
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
import test_canvas_rt_sky_ref as K
from test_canvas_rt_ref import F, H, SM, W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_skybox_ibl_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_skybox_ibl_ref.so")
_P = ctypes.c_void_p
_F3 = ctypes.c_float * 3
NO_SKY = -2                       # rsi_debug::branch_* without a sky


class RefKnobs(ctypes.Structure):
    _fields_ = [("ibl_ambient", ctypes.c_float), ("ibl_refl", ctypes.c_float), ("ibl_f0", ctypes.c_float), ("ibl_refl_mix", ctypes.c_float)]


class RefDebug(ctypes.Structure):
    _fields_ = [("branch_n", ctypes.c_int32), ("branch_r", ctypes.c_int32), ("fresnel", ctypes.c_float), ("env_n", _F3), ("env_r", _F3),
                ("refl_dir", _F3)]


class RefDebugPlanes(ctypes.Structure):
    _fields_ = [("branch_n", _P), ("branch_r", _P), ("fresnel", _P), ("env", _P)]


@functools.lru_cache(maxsize=None)
def ibl_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    for fn in (L.rsi_render, L.rsi_render_frame):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(K.RefSky), ctypes.POINTER(R.RefFrame), ctypes.POINTER(R.RefDraw), ctypes.POINTER(RefKnobs), ctypes.c_int,
                       ctypes.POINTER(R.RefPlanes), ctypes.POINTER(RefDebugPlanes)]
    L.rsi_fragments.restype = ctypes.c_int
    L.rsi_fragments.argtypes = [ctypes.POINTER(K.RefSky), ctypes.POINTER(R.RefFrame), ctypes.c_int, _P, _P, _P, ctypes.POINTER(RefKnobs), _P, _P,
                                ctypes.POINTER(RefDebug)]
    L.rsi_schlick_fresnel.restype = ctypes.c_float
    L.rsi_schlick_fresnel.argtypes = [ctypes.c_float, ctypes.c_float]
    for fn in (L.rsi_sizeof_knobs, L.rsi_sizeof_debug):
        fn.restype = ctypes.c_size_t
        fn.argtypes = []
    return L


# ---- the knobs, the skies and the frames (shared with tests/test_canvas_rt_skybox_ibl.py) ---------------------

def knobs(ibl_ambient=0.25, ibl_refl=0.35, ibl_f0=0.04, ibl_refl_mix=1.0):
    import shs_gpu
    return shs_gpu.RtSkyboxIblDraw(ibl_ambient, ibl_refl, ibl_f0, ibl_refl_mix)


def demo_knobs():
    """The demo's three sets: the floor (:1299-1302), the car (:1362-1365; here the textured quad) and the monkey (:1414-1417),
    in the order of test_canvas_rt_ref.scene_demo's draws (floor, monkey, quad)."""
    return [knobs(0.30, 0.22, 0.04, 0.10), knobs(0.30, 0.32, 0.04, 0.35), knobs(0.28, 0.38, 0.04, 0.60)]


def knobs_for(draws, sets=None):
    sets = demo_knobs() if sets is None else sets
    return [sets[i % len(sets)] for i in range(len(draws))]


# knobs below 0, inside (0, 1) and above 1; ibl_f0 0 and 1; ibl_refl_mix = 0 (the reflection vanishes, the tint stays)
EDGE_KNOBS = {
    "outside": [knobs(-0.5, 1.7, 0.04, 2.5), knobs(1.6, -0.3, 0.5, 0.7), knobs(0.6, 0.9, -0.2, -1.0)],
    "f0-0-and-1": [knobs(0.3, 1.0, 0.0, 1.0), knobs(0.3, 1.0, 1.0, 1.0), knobs(1.0, 0.5, 1.0, 0.5)],
    "no-mix": [knobs(0.8, 1.0, 0.04, 0.0), knobs(1.0, 0.7, 0.5, 0.0), knobs(0.4, 0.4, 1.0, 0.0)],
}


@functools.lru_cache(maxsize=None)
def distinct_faces(sizes=K.FACE_SIZES):
    """Faces of the sizes of test_canvas_rt_sky_ref (small, not square, all different) whose every texel is a colour of its
    own: byte channels at least 17 apart between any two texels of the cube in some channel, so that another face, a
    flipped u or v or a neighbouring texel moves a channel far beyond the tolerance."""
    n = sum(w * h for w, h in sizes)
    levels = np.arange(0, 256, 17)                                   # 16 levels per channel, 4096 colours
    rng = np.random.default_rng(77)
    pick = rng.choice(len(levels) ** 3, size=n, replace=False)
    cols = np.stack([levels[pick % 16], levels[(pick // 16) % 16], levels[pick // 256]], -1).astype(np.uint8)
    out, o = [], 0
    for w, h in sizes:
        rgba = np.full((h, w, 4), 255, np.uint8)
        rgba[..., :3] = cols[o:o + w * h].reshape(h, w, 3)
        out.append(K.Tex(rgba))
        o += w * h
    return tuple(out)


def demo_sky(which, encode=K.CLAMP):
    """'none' -> None; 'analytic': the sun low over the far end of the floor; 'cubemap': distinct_faces.  Through
    test_canvas_rt_ref's camera, under the demo's clamp encode."""
    if which == "none":
        return None
    view, _ = R.camera()
    cam = dict(fov_degrees=60.0, **K.camera_of_view(view))
    if which == "analytic":
        return K.analytic_sky(K.elevated(5.0), encode, **cam)
    return K.cubemap_sky(distinct_faces(), 1.5, encode, **cam)


SKY_NAMES = ("none", "analytic", "cubemap")


def ibl_frame(view, light_vp, w=W, h=H, tile=(160, 160), **kw):
    return R._frame(view, light_vp, w, h, tile, shading=4, **kw)


def _knobs_c(sets):
    arr = (RefKnobs * max(len(sets), 1))()
    for i, k in enumerate(sets):
        arr[i] = RefKnobs(float(k.ibl_ambient), float(k.ibl_refl), float(k.ibl_f0), float(k.ibl_refl_mix))
    return arr


def ref_render_ibl(sky, frame, draws, sets, shadow=None, background=True):
    """PASS1 of hello_ibl_skybox.cpp for a shs_gpu.RtFrame (background: with skybox_background_pass where a sky is bound)
    -> test_canvas_rt_ref.ref_render's planes and counters plus 'branch_n', 'branch_r', 'fresnel' and 'env' [.., 6]."""
    Wd, Hd = frame.width, frame.height
    keep = []
    arr = R._ref_draws(draws, keep)
    f = P._frame_c(frame, shadow, keep)
    out = {"color": np.empty((Hd, Wd, 4), np.uint8), "depth": np.empty((Hd, Wd), F), "velocity": np.empty((Hd, Wd, 2), F),
           "prequant": np.empty((Hd, Wd, 4), F), "tri_id": np.empty((Hd, Wd), np.int32), "texel": np.empty((Hd, Wd), np.int32),
           "flags": np.empty((Hd, Wd), np.int32)}
    dbg = {"branch_n": np.empty((Hd, Wd), np.int32), "branch_r": np.empty((Hd, Wd), np.int32), "fresnel": np.empty((Hd, Wd), F),
           "env": np.empty((Hd, Wd, 6), F)}
    p, g = R.RefPlanes(), RefDebugPlanes()
    for planes, c in ((out, p), (dbg, g)):
        for k, v in planes.items():
            setattr(c, k, v.ctypes.data)
    s = None if sky is None else ctypes.byref(K._sky_c(sky, keep))
    fn = ibl_lib().rsi_render_frame if background else ibl_lib().rsi_render
    assert fn(s, ctypes.byref(f), arr, _knobs_c(sets), len(draws), ctypes.byref(p), ctypes.byref(g)) == 0
    out.update(dbg)
    out["counters"] = dict(zip(("input_tris", "polys3", "polys4", "sub_tris"), (int(c) for c in p.counters)))
    return out


def ref_fragments(sky, frame, normal, world, base, sets, shadow=None):
    """fragment_shader_full :446-524 of n fragments -> (pre [n, 4], rgba [n, 4], debug: a dict of [n, ..] arrays)"""
    keep = []
    f = P._frame_c(frame, shadow, keep)
    normal, world = np.ascontiguousarray(normal, F).reshape(-1, 3), np.ascontiguousarray(world, F).reshape(-1, 3)
    n = normal.shape[0]
    base = np.ascontiguousarray(base, np.uint8).reshape(n, 3)
    pre, rgba = np.empty((n, 4), F), np.empty((n, 4), np.uint8)
    dbg = (RefDebug * max(n, 1))()
    s = None if sky is None else ctypes.byref(K._sky_c(sky, keep))
    assert ibl_lib().rsi_fragments(s, ctypes.byref(f), n, normal.ctypes.data, world.ctypes.data, base.ctypes.data, _knobs_c(sets),
                                   pre.ctypes.data, rgba.ctypes.data, dbg) == 0
    d = {"branch_n": np.array([g.branch_n for g in dbg[:n]], np.int32), "branch_r": np.array([g.branch_r for g in dbg[:n]], np.int32),
         "fresnel": np.array([g.fresnel for g in dbg[:n]], F), "env_n": np.array([list(g.env_n) for g in dbg[:n]], F).reshape(n, 3),
         "env_r": np.array([list(g.env_r) for g in dbg[:n]], F).reshape(n, 3),
         "refl_dir": np.array([list(g.refl_dir) for g in dbg[:n]], F).reshape(n, 3)}
    return pre, rgba, d


# ---- what fails without the feature, without a GPU ---------------------------------------------------------

def test_library_exports_the_entry_point_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in ("shs_rt_render_skybox_ibl", "shs_rt_render", "shs_rt_render_pbr", "shs_rt_render_pbr_soft", "shs_rt_set_sky"):
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_ctypes_knob_struct_has_the_headers_layout(tmp_path):
    """sizeof and every member's offset of shs_rt_skybox_ibl_draw against the ctypes mirror; the existing structs keep their
    sizes."""
    from shs_gpu import _abi
    names = [n for n, _ in _abi.RtSkyboxIblDrawC._fields_]
    offs = ", ".join(f"offsetof(shs_rt_skybox_ibl_draw, {n})" for n in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) {\n'
                   f'    size_t v[] = {{sizeof(shs_rt_skybox_ibl_draw), {offs}, sizeof(shs_rt_frame), sizeof(shs_rt_draw), '
                   'sizeof(shs_rt_pbr_draw), sizeof(shs_rt_sky)};\n'
                   '    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]);\n    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_abi.RtSkyboxIblDrawC)] + [getattr(_abi.RtSkyboxIblDrawC, n).offset for n in names]
    assert names == ["ibl_ambient", "ibl_refl", "ibl_f0", "ibl_refl_mix"]
    assert got[:5] == want == [16, 0, 4, 8, 12]
    assert got[5:] == [ctypes.sizeof(_abi.RtFrameC), ctypes.sizeof(_abi.RtDrawC), ctypes.sizeof(_abi.RtPbrDrawC), ctypes.sizeof(_abi.RtSkyC)] \
        == [192, 204, 60, 92]
    # the restatement's knobs are the same four floats
    assert ibl_lib().rsi_sizeof_knobs() == ctypes.sizeof(RefKnobs) == 16 and ibl_lib().rsi_sizeof_debug() == ctypes.sizeof(RefDebug)


def test_python_defaults_are_the_demos_uniforms():
    k = knobs()
    assert (k.ibl_ambient, k.ibl_refl, k.ibl_f0, k.ibl_refl_mix) == (0.25, 0.35, 0.04, 1.0)


# ---- the second restatement: float32 numpy -----------------------------------------------------------------

def _m4v(m16, p):
    """glm's mat4 * vec4(p, 1), column-major: (m0 x + m1 y) + (m2 z + m3 w)"""
    m = np.asarray(m16, F).reshape(4, 4)   # m[c][r]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return [(m[0, r] * x + m[1, r] * y) + (m[2, r] * z + m[3, r] * F(1)) for r in range(4)]


def _lround(x):
    """(int)std::lround of a product in [0, n - 1]: halves away from zero"""
    t = np.trunc(x)
    return (t + ((x - t) >= F(0.5))).astype(np.int64)


def np_shadow(frame, shadow_map, N, L, world):
    """shadow_uvz_from_world :381-399, the bias :480-481, shadow_compare :401-416 / shadow_factor_pcf_2x2 :418-440 -> [n]"""
    n = len(N)
    out = np.ones(n, F)
    if not frame.use_shadow:
        return out
    sm = np.asarray(shadow_map, F)
    sh, sw = sm.shape
    cx, cy, cz, cw = _m4v(frame.light_vp, np.asarray(world, F))
    with np.errstate(all="ignore"):
        nx, ny, z = (cx / cw).astype(F), (cy / cw).astype(F), (cz / cw).astype(F)
        called = ~(np.abs(cw) < F(1e-6)) & ~((z < 0) | (z > 1))
        u = (nx * F(0.5) + F(0.5)).astype(F)
        v = (F(1) - (ny * F(0.5) + F(0.5))).astype(F)
        ndl = P._dot(N, np.broadcast_to(L, N.shape))
        slope = F(1) - K._clamp(ndl, 0, 1)
        bias = (F(frame.bias_base) + F(frame.bias_slope) * slope).astype(F)
        fx, fy = (u * F(sw - 1)).astype(F), (v * F(sh - 1)).astype(F)
        if frame.pcf:
            x0 = np.clip(np.floor(np.nan_to_num(fx)).astype(np.int64), 0, sw - 1)
            y0 = np.clip(np.floor(np.nan_to_num(fy)).astype(np.int64), 0, sh - 1)
            x1, y1 = np.clip(x0 + 1, 0, sw - 1), np.clip(y0 + 1, 0, sh - 1)
            s = [(z <= (sm[yy, xx] + bias).astype(F)).astype(F) for xx, yy in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
            fac = (F(0.25) * (((s[0] + s[1]) + s[2]) + s[3])).astype(F)
        else:
            off = (u < 0) | (u > 1) | (v < 0) | (v > 1)
            x = np.clip(_lround(np.where(off, F(0), fx)), 0, sw - 1)
            y = np.clip(_lround(np.where(off, F(0), fy)), 0, sh - 1)
            d = sm[y, x]
            fac = np.where(off | (d == helpers.FLT_MAX), F(1), (z <= (d + bias).astype(F)).astype(F)).astype(F)
    out[called] = fac[called]
    return out


def np_fragments(sky, frame, normal, world, base, kn, shadow_map=None):
    """fragment_shader_full (hello_ibl_skybox.cpp:446-524) in float32 numpy over n fragments; kn [n, 4]: ibl_ambient,
    ibl_refl, ibl_f0, ibl_refl_mix.  -> (pre [n, 3] = (r, g, b) * 255, shadow [n], F [n], envN, envR)"""
    kn = np.asarray(kn, F)
    with np.errstate(all="ignore"):
        N = P._normalize(np.asarray(normal, F)).astype(F)
        L = P._normalize(-np.asarray(frame.light_dir_world, F)).astype(F)[None, :]
        V = P._normalize(np.asarray(frame.camera_pos, F)[None, :] - np.asarray(world, F)).astype(F)
        diff = K._gmax(P._dot(N, np.broadcast_to(L, N.shape)), F(0))
        Hh = P._normalize(L + V).astype(F)
        spec = K._powf(K._gmax(P._dot(N, Hh), F(0)), 64.0)
        specular = ((F(0.45) * spec) * F(1)).astype(F)
        col = (np.asarray(base, np.uint8).astype(F) / F(255)).astype(F)
        shadow = np_shadow(frame, shadow_map, N, L, world)
        envN, envR = np.ones_like(N), np.zeros_like(N)
        if sky is not None:
            envN = K.np_sample(sky, N)[0]
            I = -V
            R_ = (I - N * P._dot(N, I)[:, None] * F(2)).astype(F)
            envR = K.np_sample(sky, R_)[0]
        a = P._sat(kn[:, 0])[:, None]
        ambient = (F(0.18) * (np.ones_like(N) * (F(1) - a) + envN * a)).astype(F)
        NoV = K._gmax(F(0), P._dot(N, V))
        x = F(1) - P._sat(NoV)
        x2 = x * x
        x5 = x2 * x2 * x
        Fr = (kn[:, 2] + (F(1) - kn[:, 2]) * x5).astype(F)
        refl = envR * ((Fr * P._sat(kn[:, 1])) * P._sat(kn[:, 3]))[:, None]
        direct = shadow[:, None] * ((diff * F(1))[:, None] * col + specular[:, None])
        result = (ambient * col + direct) + refl
        result = K._clamp(result.astype(F), 0, 1)
        return (K._clamp(result, 0, 1) * F(255)).astype(F), shadow, Fr, envN.astype(F), envR.astype(F)


def ibl_fragments(seed=51, n=1200):
    """Normals of any length with zero and NaN ones, the cube's axes and face diagonals among them; world positions around the
    scene; random base bytes; knobs from -0.5 to 1.6, with exact 0s and 1s."""
    rng = np.random.default_rng(seed)
    normal = rng.normal(size=(n, 3)).astype(F) * rng.uniform(0.2, 3.0, (n, 1)).astype(F)
    special = np.array([(0, 0, 0), (np.nan, 0, 1), (np.nan,) * 3, (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
                        (1, 1, 0), (1, -1, 0), (0, 1, 1), (0, 1, -1), (1, 0, 1), (-1, 0, 1), (1, 1, 1), (-1, -1, -1), (1, -1, 1)], F)
    normal[:len(special) * 4] = np.tile(special, (4, 1))
    world = rng.uniform([-8, -1, -4], [8, 6, 12], (n, 3)).astype(F)
    base = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    kn = rng.uniform(-0.5, 1.6, (n, 4)).astype(F)
    kn[::7, rng.integers(0, 4)] = 0.0
    kn[3::11, rng.integers(0, 4)] = 1.0
    return normal, world, base, kn


def _sets_of(kn):
    return [knobs(*[float(v) for v in row]) for row in kn]


@pytest.mark.parametrize("use_shadow,pcf", [(True, True), (True, False), (False, True)], ids=["pcf", "compare", "no-map"])
@pytest.mark.parametrize("which", SKY_NAMES)
def test_numpy_restatement_on_random_fragments(which, use_shadow, pcf):
    view, lvp, draws = R.scene_demo()
    shadow = R.ref_shadow(SM, lvp, draws) if use_shadow else None
    sky = demo_sky(which)
    normal, world, base, kn = ibl_fragments()
    frame = ibl_frame(view, lvp, use_shadow=use_shadow, pcf=pcf)
    pre, rgba, dbg = ref_fragments(sky, frame, normal, world, base, _sets_of(kn), shadow)
    np_pre, np_shadow_f, np_F, envN, envR = np_fragments(sky, frame, normal, world, base, kn, shadow)
    assert np.array_equal(_bits(np_shadow_f), _bits(pre[:, 3])), "the shadow factor"
    assert np.array_equal(P.canonical_bits(np_F), P.canonical_bits(dbg["fresnel"])), "F"
    assert np.array_equal(P.canonical_bits(envN), P.canonical_bits(dbg["env_n"])) and np.array_equal(P.canonical_bits(envR), P.canonical_bits(dbg["env_r"]))
    bad = np.argwhere(P.canonical_bits(np_pre) != P.canonical_bits(pre[:, :3]))
    assert bad.size == 0, f"{len(bad)} of {np_pre.size} channels differ, first {bad[:4].tolist()}"
    want = np.where(np.isnan(np_pre), 0, np_pre).astype(np.uint8)       # (uint8_t) of a NaN on x86-64: 0
    assert np.array_equal(rgba[:, :3], want) and (rgba[:, 3] == 255).all()
    nan = np.isnan(pre[:, :3]).any(-1)
    assert nan.sum() >= 8 and (~nan).sum() > len(pre) - 40              # the NaN normals, and nothing else, give NaNs
    if use_shadow:
        assert len(set(pre[:, 3].tolist())) >= (3 if pcf else 2)
    if which == "cubemap":
        assert set(dbg["branch_n"].tolist()) >= set(range(6)) and set(dbg["branch_r"].tolist()) >= set(range(6))
        # a zero normal is NaN after glm::normalize: with the NaN normals it takes the cubemap's NaN path (no face is -1)
        assert np.isnan(dbg["env_n"]).all(-1).sum() >= 12 and (dbg["branch_n"] >= 0).all()
    if which == "none":
        assert (dbg["branch_n"] == NO_SKY).all() and (dbg["env_n"] == 1).all() and (dbg["env_r"] == 0).all()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- against shading 0's restatement -------------------------------------------------------------------------

def _white(draws):
    return [dataclasses.replace(d, base_color=(255, 255, 255, 255), albedo_tex=None) for d in draws]


PLANES = ("color", "depth", "velocity", "prequant", "tri_id", "texel", "flags")


def identity_cases():
    """(name, sky, knob sets): under each the shader's two additions vanish exactly."""
    zero = [knobs(0.0, 0.0, 0.04, 1.0), knobs(-0.3, -1.0, 0.9, 2.0), knobs(0.0, 0.0, 1.0, 0.0)]
    return [("no-sky", None, demo_knobs()), ("cubemap-zero-knobs", demo_sky("cubemap"), zero), ("analytic-zero-knobs", demo_sky("analytic"), zero)]


@pytest.mark.parametrize("name", ("demo",) + tuple(n for n in R.SCENES if n != "demo"))
def test_white_base_is_shading_0s_frame_bit_for_bit(name):
    """mix(1, envN, 0) = 1 exactly, refl = envR * 0 = 0, base = 255 / 255 = 1: amb + direct + refl performs shading 0's
    operations.  The background is left out (shading 0's restatement has none)."""
    view, lvp, draws = R.SCENES[name]()
    draws = _white(draws)
    shadow = R.ref_shadow(SM, lvp, draws)
    hard = R.ref_render(R._frame(view, lvp), draws, shadow)
    for case, sky, sets in identity_cases():
        got = ref_render_ibl(sky, ibl_frame(view, lvp, tile=(80, 80)), draws, knobs_for(draws, sets), shadow, background=False)
        for k in PLANES:
            a, b = got[k], hard[k]
            if k == "flags":                                             # (only shading 0's restatement records the other two bits)
                a, b = a & R.PX_NEG_AREA, b & R.PX_NEG_AREA
            same = np.array_equal(_bits(a), _bits(b)) if a.dtype == F else np.array_equal(a, b)
            assert same, f"{name}, {case}: plane {k} differs"
        assert got["counters"] == hard["counters"]
    assert (hard["tri_id"] >= 0).sum() > 1000


def test_another_base_differs_where_the_specular_term_is_not_zero():
    """The specular term does not take the base colour: with base (128, 128, 128) shading 0 gives lit * b and this shader
    (0.18 + shadow * diffuse) * b + shadow * specular, which differ by shadow * specular * (1 - b)."""
    view, lvp, draws = R.scene_demo()
    grey = [dataclasses.replace(d, base_color=(128, 128, 128, 255), albedo_tex=None) for d in draws]
    hard = R.ref_render(R._frame(view, lvp, use_shadow=False), grey)
    got = ref_render_ibl(None, ibl_frame(view, lvp, tile=(80, 80), use_shadow=False), grey, knobs_for(grey), background=False)
    white = R.ref_render(R._frame(view, lvp, use_shadow=False), _white(draws))
    for k in ("depth", "velocity", "tri_id"):
        assert np.array_equal(_bits(got[k]) if got[k].dtype == F else got[k], _bits(hard[k]) if hard[k].dtype == F else hard[k])
    shaded = hard["tri_id"] >= 0
    b = F(128) / F(255)
    d = (got["prequant"][..., 0] - hard["prequant"][..., 0]).astype(np.float64)
    # the white frame, unclamped where it is below 255, is 255 * (0.18 + diffuse + specular); specular = 0.45 * pow(.., 64) shows as
    # a highlight on the monkey: there the two shaders differ by about 255 * specular * (1 - b), elsewhere by rounding alone
    assert (d[shaded] >= -1e-3).all() and (d[shaded] > 1.0).sum() > 50
    assert (np.abs(d[shaded]) < 1e-3).sum() > 0.5 * shaded.sum()
    lit = white["prequant"][..., 0]
    assert lit[shaded & (d > 1.0)].min() > 255 * 0.18 / float(b) * 0.5


# ---- known answers -------------------------------------------------------------------------------------------

def flat_faces():
    cols = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255)]
    return tuple(K.Tex(np.tile(np.array(c + (255,), np.uint8), (h, w, 1))) for c, (w, h) in zip(cols, K.FACE_SIZES)), np.array(cols, F) / F(255)


def _one(sky, frame, n, wp, base=(255, 255, 255), k=None):
    pre, rgba, dbg = ref_fragments(sky, frame, [n], [wp], [base], [knobs() if k is None else k])
    return pre[0], rgba[0], {a: b[0] for a, b in dbg.items()}


def test_fresnel_known_answers():
    view, lvp, _ = R.scene_demo()
    frame = ibl_frame(view, lvp, use_shadow=False)
    cam = np.asarray(frame.camera_pos, np.float64)
    wp = np.array([0.0, 0.0, 3.0])
    to_cam = (cam - wp) / np.linalg.norm(cam - wp)
    for f0 in (0.0, 0.04, 0.5, 1.0):
        _, _, d = _one(None, frame, to_cam, wp, k=knobs(ibl_f0=f0))
        assert abs(float(d["fresnel"]) - f0) <= 1e-6, "facing the camera: x = 1 - N.V = 0, F = F0"
        graze = np.cross(to_cam, [0.3, 0.1, -0.5])
        _, _, d = _one(None, frame, graze, wp, k=knobs(ibl_f0=f0))
        assert abs(float(d["fresnel"]) - 1.0) <= 1e-5, "N perpendicular to V: x = 1, F = F0 + (1 - F0) = 1"
        _, _, d = _one(None, frame, -to_cam, wp, k=knobs(ibl_f0=f0))
        assert abs(float(d["fresnel"]) - 1.0) <= 1e-6, "facing away: max(0, N.V) = 0"
    assert ibl_lib().rsi_schlick_fresnel(0.04, 1.0) == F(0.04) and ibl_lib().rsi_schlick_fresnel(0.04, 0.0) == F(0.04) + (F(1) - F(0.04)) * F(1)
    assert ibl_lib().rsi_schlick_fresnel(0.25, 0.5) == F(0.25) + F(0.75) * F(0.03125)          # x = 0.5: x^5 = 1 / 32
    assert ibl_lib().rsi_schlick_fresnel(0.25, 7.0) == F(0.25) and ibl_lib().rsi_schlick_fresnel(0.25, -3.0) == F(1.0)


def test_flat_cubemap_names_the_faces_of_n_and_r():
    """Six flat colours (pure channel values: linear 0 or 1): with ibl_ambient = 1 the ambient term is 0.18 * the colour of
    N's face; with ibl_f0 = 1 (F = 1), ibl_refl = ibl_refl_mix = 1 the reflection adds the colour of R's face."""
    faces, lin = flat_faces()
    view, lvp, _ = R.scene_demo()
    sky = K.cubemap_sky(faces, 1.0, K.CLAMP, **K.camera_of_view(view))
    frame = dataclasses.replace(ibl_frame(view, lvp, use_shadow=False), light_dir_world=(0.0, 1.0, 0.0), camera_pos=(0.0, 0.0, 0.0))
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    seen, checked = set(), 0
    for fn, n in enumerate(axes):
        for fr, r in enumerate(axes):
            if fr == fn or fr == (fn ^ 1):
                continue
            # V = normalize(n - 2 r): reflect(-V, N) = 2 (N.V) N - V = (n + 2 r) / sqrt(5), which points into r's face
            nn, rr = np.array(n, np.float64), np.array(r, np.float64)
            wp = -(nn - 2.0 * rr) * 3.0            # camera at the origin: V = normalize(cam - wp)
            pre, _, d = _one(sky, frame, n, wp, base=(255, 255, 255), k=knobs(1.0, 1.0, 1.0, 1.0))
            assert np.allclose(d["refl_dir"], (nn + 2.0 * rr) / np.sqrt(5.0), atol=1e-6)
            want_r = fr
            assert d["branch_n"] == fn and d["branch_r"] == want_r
            assert np.array_equal(d["env_n"], lin[fn]) and np.array_equal(d["env_r"], lin[want_r])
            # N.L = -n.y <= 0 except for n = -y; with no diffuse and no specular: result = 0.18 * envN + envR (F = 1), clamped
            V = (nn - 2.0 * rr) / np.sqrt(5.0)
            Hh = (np.array([0.0, -1.0, 0.0]) + V) / np.linalg.norm(np.array([0.0, -1.0, 0.0]) + V)
            if n != (0, -1, 0) and float(nn @ Hh) < 0.6:                 # (0.6 ** 64 is 6e-15: no specular either)
                checked += 1
                want = np.minimum(F(0.18) * lin[fn] + lin[want_r], F(1)) * F(255)
                assert np.allclose(pre[:3], want, atol=1e-3), (n, r, pre[:3], want)
            seen.add((fn, want_r))
    assert {a for a, _ in seen} == set(range(6)) and {b for _, b in seen} == set(range(6)) and checked >= 12
    # R = reflect(-V, N) itself: V along N gives R = N; V at 45 degrees in the xy plane about N = +y gives R mirrored in x
    _, _, d = _one(sky, frame, (0, 1, 0), (0.0, -2.0, 0.0), k=knobs(1.0, 1.0, 1.0, 1.0))
    assert np.allclose(d["refl_dir"], (0, 1, 0), atol=1e-6) and d["branch_r"] == 2
    _, _, d = _one(sky, frame, (0, 1, 0), (-1.0, -1.0, 0.0), k=knobs(1.0, 1.0, 1.0, 1.0))
    assert np.allclose(d["refl_dir"], np.array([-1, 1, 0]) / np.sqrt(2), atol=1e-6)
    # ibl_refl_mix = 0: the reflection vanishes, the tint stays
    a, _, _ = _one(sky, frame, (1, 0, 0), (-3.0, 1.0, 0.5), k=knobs(1.0, 1.0, 1.0, 0.0))
    assert np.allclose(a[:3], F(0.18) * lin[0] * F(255), atol=1e-3)
    # no sky: envN = 1, envR = 0 whatever the knobs
    b, _, d = _one(None, frame, (1, 0, 0), (-3.0, 1.0, 0.5), k=knobs(1.0, 1.0, 1.0, 1.0))
    assert np.allclose(b[:3], F(0.18) * F(255), atol=1e-3) and d["branch_n"] == NO_SKY


def test_frames_cover_what_the_gpu_tests_need():
    """On the restatement alone: the demo frame under the cubemap samples every face through N or R, its tint and reflection are
    far above the tolerance, and the background fills the pixels no fragment shows."""
    view, lvp, draws = R.scene_demo()
    shadow = R.ref_shadow(SM, lvp, draws, (160, 160))
    frame = ibl_frame(view, lvp)
    sets = knobs_for(draws)
    cube = ref_render_ibl(demo_sky("cubemap"), frame, draws, sets, shadow)
    none = ref_render_ibl(None, frame, draws, sets, shadow)
    ana = ref_render_ibl(demo_sky("analytic"), frame, draws, sets, shadow)
    shaded = cube["tri_id"] >= 0
    assert shaded.sum() > 0.5 * W * H and (~shaded).sum() > 2000
    assert set(np.unique(cube["branch_n"][shaded])) | set(np.unique(cube["branch_r"][shaded])) >= set(range(6))
    for other in (cube, ana):
        d = np.abs(other["prequant"][..., :3] - none["prequant"][..., :3]).max(-1)
        assert (d[shaded] > 100 * helpers.TOL * 255).mean() > 0.9
        assert (other["color"][~shaded] != np.array(frame.clear_color, np.uint8)).any(-1).mean() > 0.99
        for k in ("depth", "velocity", "tri_id"):
            assert np.array_equal(other[k], none[k])
    assert (none["color"][~shaded] == np.array(frame.clear_color, np.uint8)).all()
    vals = set(np.unique(cube["prequant"][..., 3][shaded]).tolist())
    assert vals == {0.0, 0.25, 0.5, 0.75, 1.0}, vals
    # a neighbouring texel of the cubemap would show: any two texels of a face differ by at least 17 in some byte channel
    for t in distinct_faces():
        c = t.rgba[..., :3].reshape(-1, 3).astype(int)
        if len(c) > 1:
            dist = np.abs(c[:, None, :] - c[None, :, :]).max(-1)
            assert dist[~np.eye(len(c), dtype=bool)].min() >= 17
