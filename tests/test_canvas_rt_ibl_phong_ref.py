"""tests/canvas_rt_ibl_phong_ref (ref_canvas_rt_ibl_phong.c), the C restatement of what hello_ibl_skybox_optimized.cpp and
hello_ibl_skybox_xsimd.cpp have that the other demos do not -- their fragment_shader_full (optimized :875-958: Blinn-Phong
with a per-object shininess, an irradiance cubemap and a prefiltered-specular mip chain) behind the hard demo's raster, and
the xsimd demo's edge-function shadow raster (xsimd :1016-1191) -- the reference of tests/test_canvas_rt_ibl_phong.py,
pinned on the CPU:

  * against a second restatement of the shader in float32 numpy, written from the same cited lines, on seeded random
    fragments and on every shown pixel of the existing scenes (scene_demo, the edge scenes of test_canvas_rt_edges_ref);
  * against a second restatement of the edge raster in float32 numpy on the scenes of EDGE_SCENES;
  * by known answers of the shader (shininess 0, ibl_f0 = 1, a one-colour IBL, an IBL whose every texel is a colour of its
    own, no IBL) and of the raster (a light-facing triangle against its mirror image, a triangle left of the map);
  * by rule swaps: each rule of the two, replaced by a plausible other one, changes texels or pixels of a named scene;
  * with the ABI struct's size and offsets against the ctypes mirror.

It also holds the wrapper, the knob sets, the IBL and the scenes the GPU test shares, and what fails without the feature
and needs no GPU: the new entry points and the struct."""
import ctypes
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers
import test_canvas_rt_edges_ref as E
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
import test_canvas_rt_sky_ref as K
import test_canvas_rt_skybox_ibl_ref as I
from test_canvas_rt_ref import F, H, SM, W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_ibl_phong_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_ibl_phong_ref.so")
_P = ctypes.c_void_p
FLT_MAX = helpers.FLT_MAX
EYE = np.eye(4, dtype=F).reshape(16)

# ref_canvas_rt_ibl_phong.c's RIP_SWAP_*
SWAP_FIXED_LOD, SWAP_POW64, SWAP_SHADOW_ON_IBL = 1, 2, 4
SWAP_BODY, SWAP_TAIL, SWAP_STRICT, SWAP_BC, SWAP_NO_CULL, SWAP_NO_CEIL = 16, 32, 64, 128, 256, 512


class RefKnobs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("ibl_ambient", "ibl_refl", "ibl_f0", "ibl_refl_mix", "shininess")]


class RefDebug(ctypes.Structure):
    _fields_ = [("face_n", ctypes.c_int32), ("face_r", ctypes.c_int32), ("m0", ctypes.c_int32), ("m1", ctypes.c_int32),
                ("lod", ctypes.c_float), ("fresnel", ctypes.c_float), ("spec", ctypes.c_float)]


class RefDebugPlanes(ctypes.Structure):
    _fields_ = [("face_n", _P), ("face_r", _P), ("m0", _P), ("lod", _P), ("spec", _P), ("frag_in", _P), ("base", _P)]


@functools.lru_cache(maxsize=None)
def phong_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    L.rip_render.restype = ctypes.c_int
    L.rip_render.argtypes = [ctypes.POINTER(P.RefIbl), ctypes.POINTER(R.RefFrame), ctypes.POINTER(R.RefDraw), ctypes.POINTER(RefKnobs),
                             ctypes.c_int, ctypes.c_int, ctypes.POINTER(R.RefPlanes), ctypes.POINTER(RefDebugPlanes)]
    L.rip_render_frame.restype = ctypes.c_int
    L.rip_render_frame.argtypes = [ctypes.POINTER(K.RefSky)] + L.rip_render.argtypes
    L.rip_fragments.restype = ctypes.c_int
    L.rip_fragments.argtypes = [ctypes.POINTER(P.RefIbl), ctypes.POINTER(R.RefFrame), ctypes.c_int, _P, _P, _P, ctypes.POINTER(RefKnobs),
                                ctypes.c_int, _P, _P, ctypes.POINTER(RefDebug)]
    L.rip_render_shadow_edge.restype = ctypes.c_int
    L.rip_render_shadow_edge.argtypes = [ctypes.c_int] * 6 + [_P, ctypes.POINTER(R.RefDraw), ctypes.c_int, _P, _P]
    for fn in (L.rip_sizeof_knobs, L.rip_sizeof_debug):
        fn.restype = ctypes.c_size_t
        fn.argtypes = []
    return L


# ---- the knobs, the IBL and the frames (shared with tests/test_canvas_rt_ibl_phong.py) ---------------------------

def knobs(ibl_ambient=0.30, ibl_refl=0.35, ibl_f0=0.04, ibl_refl_mix=1.0, shininess=64.0):
    import shs_gpu
    return shs_gpu.RtIblPhongDraw(ibl_ambient, ibl_refl, ibl_f0, ibl_refl_mix, shininess)


def demo_knobs():
    """The demo's three sets: the floor (optimized :1737-1741), the car (:1805-1809; here the textured quad) and the monkey
    (:1862-1866), in the order of test_canvas_rt_ref.scene_demo's draws (floor, monkey, quad)."""
    return [knobs(0.30, 0.20, 0.04, 0.08, 32.0), knobs(0.30, 0.28, 0.04, 0.35, 48.0), knobs(0.28, 0.45, 0.04, 0.70, 96.0)]


def knobs_for(draws, sets=None):
    sets = demo_knobs() if sets is None else sets
    return [sets[i % len(sets)] for i in range(len(draws))]


SHININESS = (0.0, 1.0, 32.0, 48.0, 96.0, 2.5, 1000.0)


@functools.lru_cache(maxsize=None)
def distinct_ibl(irr_size=4, spec_base=8, mips=4):
    """An IBL whose every texel, of the irradiance map and of every specular mip, is a colour of its own: channels on a
    lattice of 16 levels in [0, 2], any two texels at least 2 / 15 apart in some channel, so that another face, mip or
    texel moves a channel far beyond the tolerance.  The sizes have a size-1 level, as test_canvas_rt_pbr_ref.make_ibl's."""
    sizes = [irr_size] + [max(1, spec_base >> m) for m in range(mips)]
    n = sum(6 * s * s for s in sizes)
    rng = np.random.default_rng(177)
    pick = rng.choice(16 ** 3, size=n, replace=False)
    cols = (np.stack([pick % 16, (pick // 16) % 16, pick // 256], -1).astype(F) * F(2.0 / 15.0)).astype(F)
    out, o = [], 0
    for s in sizes:
        out.append(np.ascontiguousarray(cols[o:o + 6 * s * s].reshape(6, s, s, 3)))
        o += 6 * s * s
    return out[0], tuple(out[1:])


def one_colour_ibl(rgb=(0.5, 1.0, 0.25), irr_size=4, spec_base=8, mips=4):
    c = np.asarray(rgb, F)
    lvl = lambda s: np.ascontiguousarray(np.broadcast_to(c, (6, s, s, 3)))   # noqa: E731
    return lvl(irr_size), tuple(lvl(max(1, spec_base >> m)) for m in range(mips))


def phong_frame(view, light_vp, w=W, h=H, tile=(160, 160), **kw):
    return R._frame(view, light_vp, w, h, tile, shading=11, **kw)


def _knobs_c(sets):
    arr = (RefKnobs * max(len(sets), 1))()
    for i, k in enumerate(sets):
        arr[i] = RefKnobs(float(k.ibl_ambient), float(k.ibl_refl), float(k.ibl_f0), float(k.ibl_refl_mix), float(k.shininess))
    return arr


def ref_render_phong(ibl, frame, draws, sets, shadow=None, sky=None, swaps=0):
    """PASS1 of the two demos for a shs_gpu.RtFrame (with skybox_background_pass where a sky is given) ->
    test_canvas_rt_ref.ref_render's planes and counters plus 'face_n', 'face_r', 'm0', 'lod', 'spec', 'frag_in' [.., 6] and
    'base' [.., 3]."""
    Wd, Hd = frame.width, frame.height
    keep = []
    arr = R._ref_draws(draws, keep)
    f = P._frame_c(frame, shadow, keep)
    out = {"color": np.empty((Hd, Wd, 4), np.uint8), "depth": np.empty((Hd, Wd), F), "velocity": np.empty((Hd, Wd, 2), F),
           "prequant": np.empty((Hd, Wd, 4), F), "tri_id": np.empty((Hd, Wd), np.int32), "texel": np.empty((Hd, Wd), np.int32),
           "flags": np.empty((Hd, Wd), np.int32)}
    dbg = {"face_n": np.empty((Hd, Wd), np.int32), "face_r": np.empty((Hd, Wd), np.int32), "m0": np.empty((Hd, Wd), np.int32),
           "lod": np.empty((Hd, Wd), F), "spec": np.empty((Hd, Wd), F), "frag_in": np.empty((Hd, Wd, 6), F),
           "base": np.empty((Hd, Wd, 3), np.uint8)}
    p, g = R.RefPlanes(), RefDebugPlanes()
    for planes, c in ((out, p), (dbg, g)):
        for k, v in planes.items():
            setattr(c, k, v.ctypes.data)
    ic = P._ibl_c(ibl, keep)
    ip = None if ic is None else ctypes.byref(ic)
    s = None if sky is None else ctypes.byref(K._sky_c(sky, keep))
    assert phong_lib().rip_render_frame(s, ip, ctypes.byref(f), arr, _knobs_c(sets), len(draws), swaps, ctypes.byref(p), ctypes.byref(g)) == 0
    out.update(dbg)
    out["counters"] = dict(zip(("input_tris", "polys3", "polys4", "sub_tris"), (int(c) for c in p.counters)))
    return out


def ref_fragments(ibl, frame, normal, world, base, sets, shadow=None, swaps=0):
    """fragment_shader_full of n fragments -> (pre [n, 4], rgba [n, 4], debug: a dict of [n] arrays)"""
    keep = []
    f = P._frame_c(frame, shadow, keep)
    normal, world = np.ascontiguousarray(normal, F).reshape(-1, 3), np.ascontiguousarray(world, F).reshape(-1, 3)
    n = normal.shape[0]
    base = np.ascontiguousarray(base, np.uint8).reshape(n, 3)
    pre, rgba = np.empty((n, 4), F), np.empty((n, 4), np.uint8)
    dbg = (RefDebug * max(n, 1))()
    ic = P._ibl_c(ibl, keep)
    assert phong_lib().rip_fragments(None if ic is None else ctypes.byref(ic), ctypes.byref(f), n, normal.ctypes.data, world.ctypes.data,
                                     base.ctypes.data, _knobs_c(sets), swaps, pre.ctypes.data, rgba.ctypes.data, dbg) == 0
    d = {k: np.array([getattr(g, k) for g in dbg[:n]], t) for k, t in (("face_n", np.int32), ("face_r", np.int32), ("m0", np.int32),
                                                                        ("m1", np.int32), ("lod", F), ("fresnel", F), ("spec", F))}
    return pre, rgba, d


def ref_shadow_edge(size, light_vp, casters, tile=(160, 160), lanes=8, swaps=0, visits=False):
    """PASS0 of hello_ibl_skybox_xsimd.cpp -> the shadow map float32 [h, w] (y down); visits: also how often the loops
    reached each texel."""
    w, h = (size, size) if isinstance(size, int) else size
    keep = []
    arr = R._ref_draws(casters, keep)
    lvp = np.ascontiguousarray(light_vp, F).reshape(16)
    sm = np.empty((h, w), F)
    vis = np.empty((h, w), np.int32) if visits else None
    assert phong_lib().rip_render_shadow_edge(w, h, tile[0], tile[1], lanes, swaps, lvp.ctypes.data, arr, len(casters), sm.ctypes.data,
                                              None if vis is None else vis.ctypes.data) == 0
    return (sm, vis) if visits else sm


# ---- the edge raster's scenes (shared with the GPU test) ---------------------------------------------------------

def _caster(tris, model=EYE):
    import shs_gpu
    return shs_gpu.RtDraw(R.SoupMesh(np.asarray(tris, F).reshape(-1, 9)), np.asarray(model, F), EYE, EYE, (200, 200, 200, 255), None)


def texel_light(n):
    """An orthographic light_vp under which world (x, y) is texel (x, y) of an n x n map, y down, but for the rounding of its
    operations, and world z in [0, 1] is the depth."""
    return R.ortho_lh_zo(0.0, float(n - 1), float(n - 1), 0.0, 0.0, 1.0)


def scene_mirror(n=50):
    """A triangle that faces the light and its mirror image (the same corners in the other order) beside it, nearer."""
    front = [5.0, 5.0, 0.5, 20.0, 5.0, 0.5, 5.0, 30.0, 0.5]
    back = [25.0, 5.0, 0.25, 25.0, 30.0, 0.25, 40.0, 5.0, 0.25]
    return texel_light(n), [_caster([front]), _caster([back])]


def scene_left_of_map(n=50):
    """A triangle wholly left of the map: its box is clamped to column 0, where every edge rejects it."""
    return texel_light(n), [_caster([[-30.0, 5.0, 0.5, -10.0, 5.0, 0.5, -30.0, 30.0, 0.5]])]


THIRDS_SEED = 5


def scene_thirds(n=50, seed=THIRDS_SEED, count=24):
    """The constructed scene of the association tests: triangles whose corners lie at thirds of a texel (not representable)
    with one edge along a line x + y = c + 1 through texel centres, under texel_light, at seeded depths."""
    rng = np.random.default_rng(seed)
    tris = []
    for _ in range(count):
        x0, y0 = rng.integers(1, n - 16, 2)
        a, b = rng.integers(4, 14, 2)
        t = float(rng.integers(0, 3)) / 3.0
        z = rng.uniform(0.1, 0.9, 3)
        # the hypotenuse from (x0 + a + 0.5 + t, y0 + 0.5 - t) to (x0 + 0.5 - t, y0 + a + 0.5 + t) passes through the centres
        # (x0 + k + 0.5, y0 + a - k + 0.5); the third corner at a third
        p0 = (x0 + 0.5 - t - b / 3.0, y0 + 0.5 - t - b / 3.0, z[0])
        p1 = (x0 + 0.5 - t, y0 + a + 0.5 + t, z[1])
        p2 = (x0 + a + 0.5 + t, y0 + 0.5 - t, z[2])
        tris.append(np.array(p0 + p2 + p1, np.float64))          # (positive area on the map, y down)
    return texel_light(n), [_caster(np.array(tris, F))]


def scene_random(seed, n=50, count=60):
    """Seeded triangles of both windings around and across the map's edges, depths from below 0 to above 1."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-8, n + 8, (count, 1, 2))
    p = c + rng.normal(size=(count, 3, 2)) * rng.uniform(0.3, 14, (count, 1, 1))
    z = rng.uniform(-0.15, 1.15, (count, 3, 1))
    return texel_light(n), [_caster(np.concatenate([p, z], -1).reshape(count, 9))]


def scene_nonfinite_casters(n=50):
    """Corners that are NaN, infinite or beyond an int on the screen (dropped), w = 0 (dropped), and two ordinary ones."""
    ok = [3.0, 3.0, 0.5, 20.0, 3.0, 0.5, 3.0, 20.0, 0.5]
    big = [3.0, 3.0, 0.5, 4e9, 3.0, 0.5, 3.0, 4e9, 0.5]
    nan = [np.nan, 3.0, 0.5, 20.0, 3.0, 0.5, 3.0, 20.0, 0.5]
    inf = [3.0, 3.0, 0.5, 20.0, 3.0, 0.5, 3.0, np.inf, 0.5]
    wide = [-3e5, 8.0, 0.3, 3e5, 8.0, 0.3, 8.0, 3e5, 0.3]          # huge and inside int: drawn
    # under the model NEAR_M the clip w is z + 1: a corner at z = -1 has w = 0
    return texel_light(n), [_caster([ok, big, nan, inf, wide]), _caster([[3.0, 3.0, -1.0, 20.0, 3.0, 0.5, 3.0, 20.0, 0.5]], model=R.NEAR_M),
                            _caster([[25.0, 25.0, 0.7, 45.0, 25.0, 0.7, 25.0, 45.0, 0.7]])]


def _named(fn):
    def scene():
        _, lvp, draws = fn()
        return lvp, draws
    return scene


EDGE_SCENES = {
    "demo": _named(R.scene_demo), "windings": _named(R.scene_windings), "near": _named(R.scene_near),
    "coincident": _named(R.scene_coincident), "outside_light": _named(R.scene_outside_light),
    "perspective_light": lambda: (E.perspective_light(), R.scene_demo()[2]),
    "mirror": scene_mirror, "left_of_map": scene_left_of_map, "thirds": scene_thirds, "nonfinite": scene_nonfinite_casters,
    "random1": lambda: scene_random(1), "random2": lambda: scene_random(2), "random3": lambda: scene_random(3),
    "random4": lambda: scene_random(4),
}
EDGE_TILES = [(160, 160), (64, 48), (7, 5)]
EDGE_LANES = [1, 4, 8, 16]
EDGE_MAPS = [8, 50, 96]


def _bits(a):
    return P.canonical_bits(a)


# ---- what fails without the feature, without a GPU ---------------------------------------------------------

def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in ("shs_rt_render_ibl_phong", "shs_rt_render_shadow_edge", "shs_rt_render_shadow", "shs_rt_render", "shs_rt_set_ibl"):
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_ctypes_knob_struct_has_the_headers_layout(tmp_path):
    """sizeof and every member's offset of shs_rt_ibl_phong_draw against the ctypes mirror; the existing structs keep their
    sizes."""
    from shs_gpu import _abi
    names = [n for n, _ in _abi.RtIblPhongDrawC._fields_]
    offs = ", ".join(f"offsetof(shs_rt_ibl_phong_draw, {n})" for n in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) {\n'
                   f'    size_t v[] = {{sizeof(shs_rt_ibl_phong_draw), {offs}, sizeof(shs_rt_frame), sizeof(shs_rt_draw), '
                   'sizeof(shs_rt_skybox_ibl_draw)};\n'
                   '    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]);\n    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_abi.RtIblPhongDrawC)] + [getattr(_abi.RtIblPhongDrawC, n).offset for n in names]
    assert names == ["ibl_ambient", "ibl_refl", "ibl_f0", "ibl_refl_mix", "shininess"]
    assert got[:6] == want == [20, 0, 4, 8, 12, 16]
    assert got[6:] == [ctypes.sizeof(_abi.RtFrameC), ctypes.sizeof(_abi.RtDrawC), ctypes.sizeof(_abi.RtSkyboxIblDrawC)] == [192, 204, 16]
    assert phong_lib().rip_sizeof_knobs() == ctypes.sizeof(RefKnobs) == 20 and phong_lib().rip_sizeof_debug() == ctypes.sizeof(RefDebug)


def test_python_defaults_are_the_demos_uniforms():
    k = knobs()
    assert (k.ibl_ambient, k.ibl_refl, k.ibl_f0, k.ibl_refl_mix, k.shininess) == (0.30, 0.35, 0.04, 1.0, 64.0)


# ---- the second restatement of the shader: float32 numpy -------------------------------------------------------

def _powf2(x, e):
    """libm's powf, element by element, the function the C restatement calls"""
    p = K._libm().powf
    x, e = np.broadcast_arrays(np.asarray(x, F), np.asarray(e, F))
    return np.array([p(float(a), float(b)) for a, b in zip(x.ravel(), e.ravel())], F).reshape(x.shape)


def np_fragments(ibl, frame, normal, world, base, kn, shadow_map=None):
    """fragment_shader_full (optimized :875-958) in float32 numpy over n fragments with finite, non-zero normals; kn [n, 5]:
    ibl_ambient, ibl_refl, ibl_f0, ibl_refl_mix, shininess.  -> (pre [n, 3] = (r, g, b) * 255, shadow [n], lod [n])"""
    kn = np.asarray(kn, F)
    with np.errstate(all="ignore"):
        N = P._normalize(np.asarray(normal, F)).astype(F)
        L = P._normalize(-np.asarray(frame.light_dir_world, F)).astype(F)[None, :]
        V = P._normalize(np.asarray(frame.camera_pos, F)[None, :] - np.asarray(world, F)).astype(F)
        diff = K._gmax(P._dot(N, np.broadcast_to(L, N.shape)), F(0))
        Hh = P._normalize(L + V).astype(F)
        spec = _powf2(K._gmax(P._dot(N, Hh), F(0)), kn[:, 4])
        specular = ((F(0.45) * spec) * F(1)).astype(F)
        col = (np.asarray(base, np.uint8).astype(F) / F(255)).astype(F)
        shadow = I.np_shadow(frame, shadow_map, N, L, world)
        idiff, ispec = np.zeros_like(N), np.zeros_like(N)
        lod = np.zeros(len(N), F)
        if ibl is not None:
            irr_map, spec_maps = ibl
            irr = P.np_cube(irr_map, N)[0]
            rough = np.sqrt(F(2) / (kn[:, 4] + F(2))).astype(F)
            lod = (rough * F(len(spec_maps) - 1)).astype(F)
            Iv = -V
            R_ = (Iv - N * P._dot(N, Iv)[:, None] * F(2)).astype(F)
            pre = P.np_trilinear(list(spec_maps), R_, lod)[0]
            NoV = K._gmax(F(0), P._dot(N, V))
            x = F(1) - P._sat(NoV)
            x2 = x * x
            x5 = x2 * x2 * x
            Fr = (kn[:, 2] + (F(1) - kn[:, 2]) * x5).astype(F)
            kd = (F(1) - Fr).astype(F)
            idiff = ((kd[:, None] * irr) * P._sat(kn[:, 0])[:, None]).astype(F)
            ispec = (((Fr[:, None] * pre) * P._sat(kn[:, 1])[:, None]) * P._sat(kn[:, 3])[:, None]).astype(F)
        direct = (shadow[:, None] * ((diff * F(1))[:, None] * col + specular[:, None])).astype(F)
        amb = (F(0.18) * col).astype(F)
        result = (((amb + direct) + idiff * col) + ispec).astype(F)
        result = K._clamp(result, 0, 1)
        return (K._clamp(result, 0, 1) * F(255)).astype(F), shadow, lod


def phong_fragments(seed=61, n=900):
    """Finite normals of any length, the cube's axes and face diagonals among them; world positions around the scene; random
    base bytes; knobs from -0.5 to 1.6 with exact 0s and 1s; shininess among SHININESS and seeded values up to 300."""
    rng = np.random.default_rng(seed)
    normal = rng.normal(size=(n, 3)).astype(F) * rng.uniform(0.2, 3.0, (n, 1)).astype(F)
    special = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, -1, 0), (0, 1, 1), (0, 1, -1),
                        (1, 0, 1), (-1, 0, 1), (1, 1, 1), (-1, -1, -1), (1, -1, 1)], F)
    normal[:len(special) * 4] = np.tile(special, (4, 1))
    world = rng.uniform([-8, -1, -4], [8, 6, 12], (n, 3)).astype(F)
    base = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    kn = np.empty((n, 5), F)
    kn[:, :4] = rng.uniform(-0.5, 1.6, (n, 4))
    kn[::7, rng.integers(0, 4)] = 0.0
    kn[3::11, rng.integers(0, 4)] = 1.0
    kn[:, 4] = rng.uniform(0.0, 300.0, n)
    kn[::3, 4] = np.asarray(SHININESS, F)[rng.integers(0, len(SHININESS), len(kn[::3]))]
    return normal, world, base, kn


def _sets_of(kn):
    return [knobs(*[float(v) for v in row]) for row in kn]


@pytest.mark.parametrize("use_shadow,pcf", [(True, True), (True, False), (False, True)], ids=["pcf", "compare", "no-map"])
@pytest.mark.parametrize("which", ["distinct", "random", "none"])
def test_numpy_restatement_on_random_fragments(which, use_shadow, pcf):
    view, lvp, draws = R.scene_demo()
    shadow = R.ref_shadow(SM, lvp, draws) if use_shadow else None
    ibl = {"distinct": distinct_ibl(), "random": P.make_ibl(3, 5, 6, 3), "none": None}[which]
    normal, world, base, kn = phong_fragments()
    frame = phong_frame(view, lvp, use_shadow=use_shadow, pcf=pcf)
    pre, rgba, dbg = ref_fragments(ibl, frame, normal, world, base, _sets_of(kn), shadow)
    np_pre, np_shadow_f, np_lod = np_fragments(ibl, frame, normal, world, base, kn, shadow)
    assert np.array_equal(_bits(np_shadow_f), _bits(pre[:, 3])), "the shadow factor"
    assert np.array_equal(_bits(np_lod), _bits(dbg["lod"])), "the lod"
    bad = np.argwhere(_bits(np_pre) != _bits(pre[:, :3]))
    assert bad.size == 0, f"{len(bad)} of {np_pre.size} channels differ, first {bad[:4].tolist()}"
    assert np.array_equal(rgba[:, :3], np_pre.astype(np.uint8)) and (rgba[:, 3] == 255).all() and not np.isnan(pre).any()
    if use_shadow:
        assert len(set(pre[:, 3].tolist())) >= (3 if pcf else 2)
    if ibl is not None:
        assert set(dbg["face_n"].tolist()) >= set(range(6)) and set(dbg["face_r"].tolist()) >= set(range(6))
        assert set(dbg["m0"].tolist()) >= set(range(len(ibl[1]) - 1))
    else:
        assert (dbg["face_n"] == -1).all() and (dbg["lod"] == 0).all()


def shader_scenes():
    """The existing scenes the shader runs on: (name, view, lvp, draws, frame options)."""
    out = [("demo",) + R.scene_demo() + ({},)]
    for name in E.SHADING_NAMES:
        out.append((name,) + tuple(E.shading_scene(name)))
    return out


@pytest.mark.parametrize("name", ["demo"] + E.SHADING_NAMES)
def test_numpy_restatement_on_every_pixel_of_the_scenes(name):
    _, view, lvp, draws, opts = next(s for s in shader_scenes() if s[0] == name)
    opts = dict(opts)
    shadow = R.ref_shadow(opts.pop("sm", SM), lvp, draws, (160, 160))
    frame = phong_frame(view, lvp, **opts)
    sets = knobs_for(draws)
    ibl = distinct_ibl()
    ref = ref_render_phong(ibl, frame, draws, sets, shadow if frame.use_shadow else None)
    px = ref["tri_id"] >= 0
    fi = ref["frag_in"][px]
    fin = np.isfinite(fi).all(-1) & (np.abs(fi[:, :3]).max(-1) > 0)
    assert fin.sum() > 100
    ends = np.cumsum([d.mesh.positions.shape[0] for d in draws])
    who = np.searchsorted(ends, ref["tri_id"][px] // 2, side="right")
    kn = np.array([[k.ibl_ambient, k.ibl_refl, k.ibl_f0, k.ibl_refl_mix, k.shininess] for k in sets], F)[who]
    np_pre, np_sh, _ = np_fragments(ibl, frame, fi[fin, :3], fi[fin, 3:], ref["base"][px][fin], kn[fin], shadow if frame.use_shadow else None)
    got = ref["prequant"][px][fin]
    assert np.array_equal(_bits(np_sh), _bits(got[:, 3]))
    both = np.isfinite(np_pre).all(-1) & np.isfinite(got[:, :3]).all(-1)
    assert both.sum() > 100 and np.array_equal(np.isfinite(np_pre).all(-1), np.isfinite(got[:, :3]).all(-1))
    bad = np.argwhere(_bits(np_pre[both]) != _bits(got[both][:, :3]))
    assert bad.size == 0, f"{name}: {len(bad)} of {np_pre[both].size} channels differ, first {bad[:4].tolist()}"


# ---- known answers of the shader ---------------------------------------------------------------------------------

def _plain_frame(**kw):
    view, lvp, _ = R.scene_demo()
    return phong_frame(view, lvp, use_shadow=False, **kw)


def test_shader_known_answers():
    frame = _plain_frame()
    normal, world, base, kn = phong_fragments(seed=62, n=300)
    # shininess = 0: pow(., 0) = 1, so the specular term is 0.45 whatever N.H is, a zero N.H included
    kn0 = kn.copy()
    kn0[:, 4] = 0.0
    _, _, d = ref_fragments(None, frame, normal, world, base, _sets_of(kn0))
    assert (d["spec"] == 1.0).all()
    pre, _, _ = ref_fragments(None, frame, normal, world, np.zeros_like(base), _sets_of(kn0))     # a black base: the specular term alone
    assert np.array_equal(pre[:, :3], np.broadcast_to(F(F(0.45) * F(255)), (len(pre), 3)))
    # no IBL bound: the direct and ambient terms alone -- the knobs but the shininess do nothing
    a, _, da = ref_fragments(None, frame, normal, world, base, _sets_of(kn))
    knz = kn.copy()
    knz[:, :4] = 0.0
    b, _, _ = ref_fragments(None, frame, normal, world, base, _sets_of(knz))
    assert np.array_equal(_bits(a), _bits(b)) and (da["face_n"] == -1).all() and (da["m0"] == -1).all()
    # ... and with a white base that is shading 0's shader but for the exponent: at 64 the same floats
    k64 = kn.copy()
    k64[:, 4] = 64.0
    white = np.full_like(base, 255)
    c, _, _ = ref_fragments(None, frame, normal, world, white, _sets_of(k64))
    e, _, _ = I.ref_fragments(None, dataclasses.replace(frame, shading=4), normal, world, white, [I.knobs(0.0, 0.0, 0.04, 0.0)] * len(kn))
    assert np.array_equal(_bits(c), _bits(e))
    # a one-colour IBL, f0 = 1 (F = 1: kd = 0, ks = 1), a black base, no light from the front: the colour times refl * mix
    col = np.array([0.5, 1.0, 0.25], F)
    one = one_colour_ibl(col)
    kf = kn.copy()
    kf[:, 2], kf[:, 1], kf[:, 3], kf[:, 4] = 1.0, 0.5, 0.5, 1000.0
    g, _, dg = ref_fragments(one, frame, normal, world, np.zeros_like(base), _sets_of(kf))
    assert (dg["fresnel"] == 1.0).all()
    lit = dg["spec"] == 0.0                                                    # pow(., 1000) underflows off the highlight
    assert lit.sum() > 200
    assert np.array_equal(g[lit][:, :3], np.broadcast_to(((col * F(0.5)) * F(0.5)) * F(255), (int(lit.sum()), 3)).astype(F))
    # f0 = 1 and a white base without direct light: kd = 0 removes the irradiance term whatever ibl_ambient is
    h1, _, _ = ref_fragments(one, frame, normal, world, white, _sets_of(kf))
    kg = kf.copy()
    kg[:, 0] = 0.0
    h2, _, _ = ref_fragments(one, frame, normal, world, white, _sets_of(kg))
    assert np.array_equal(_bits(h1), _bits(h2))
    # f0 = 0 facing the camera would be kd = 1; with f0 = 0, refl = 0: amb + direct + kd * colour * ambient * base
    kd_ = kn.copy()
    kd_[:, 2], kd_[:, 1], kd_[:, 0] = 0.0, 0.0, 1.0
    q, _, dq = ref_fragments(one, frame, normal, world, white, _sets_of(kd_))
    w0, _, _ = ref_fragments(None, frame, normal, world, white, _sets_of(kd_))
    kdv = (F(1) - dq["fresnel"]).astype(F)
    want = K._clamp((w0[:, :3] / F(255) + ((kdv[:, None] * col[None, :]) * F(1)) * F(1)).astype(F), 0, 1) * F(255)
    unsat = (w0[:, :3] < 255).all(-1) & (want < 255).all(-1)
    assert unsat.sum() > 50 and np.abs(q[unsat][:, :3] - want[unsat]).max() < 1e-3
    # the lod: sqrt(2 / (s + 2)) * (mips - 1); shininess 0 is the last mip, 1000 close to the first
    for s, lod in ((0.0, 3.0), (2.0 * 9 - 2, 1.0), (1000.0, float(F(np.sqrt(F(2) / F(1002))) * F(3)))):
        ks_ = kn.copy()
        ks_[:, 4] = s
        _, _, dl = ref_fragments(distinct_ibl(), frame, normal, world, base, _sets_of(ks_))
        assert (dl["lod"] == F(lod)).all() and (dl["m0"] == int(lod)).all()


def test_distinct_ibl_names_its_texels():
    irr, spec = distinct_ibl()
    flat = np.concatenate([irr.reshape(-1, 3)] + [m.reshape(-1, 3) for m in spec])
    assert len(np.unique(flat, axis=0)) == len(flat) == 6 * (16 + 64 + 16 + 4 + 1)
    d = np.abs(flat[:, None, :] - flat[None, :, :]).max(-1)
    assert d[~np.eye(len(flat), dtype=bool)].min() >= 2.0 / 15.0 - 1e-6
    # the shader on an axis: irradiance texel (face, centre) -- the four centre texels' mix -- reaches the colour
    frame = _plain_frame()
    n = np.array([[0, 1, 0]], F)
    wp = np.array([[0, 0, 0]], F)
    pre, _, d = ref_fragments((irr, spec), frame, n, wp, np.full((1, 3), 255, np.uint8), [knobs(1.0, 0.0, 0.0, 0.0, 64.0)])
    off, _, _ = ref_fragments(None, frame, n, wp, np.full((1, 3), 255, np.uint8), [knobs(1.0, 0.0, 0.0, 0.0, 64.0)])
    assert d["face_n"][0] == 2 and (pre[0, :3] >= off[0, :3]).all() and (pre[0, :3] != off[0, :3]).any()


# ---- rule swaps of the shader: each changes pixels of the demo scene ----------------------------------------------

@pytest.mark.parametrize("swap,name", [(SWAP_FIXED_LOD, "lod from a fixed shininess"), (SWAP_POW64, "pow64 in place of the variable exponent"),
                                       (SWAP_SHADOW_ON_IBL, "shadow applied to the IBL terms")])
def test_shader_rule_swaps_change_the_demo_frame(swap, name):
    view, lvp, draws = R.scene_demo()
    shadow = R.ref_shadow(SM, lvp, draws, (160, 160))
    frame = phong_frame(view, lvp)
    ref = ref_render_phong(distinct_ibl(), frame, draws, knobs_for(draws), shadow)
    other = ref_render_phong(distinct_ibl(), frame, draws, knobs_for(draws), shadow, swaps=swap)
    for k in ("tri_id", "depth", "velocity"):
        assert np.array_equal(_bits(ref[k]) if ref[k].dtype == F else ref[k], _bits(other[k]) if other[k].dtype == F else other[k])
    moved = np.abs(ref["prequant"][..., :3] - other["prequant"][..., :3]).max(-1) > 100 * helpers.TOL * 255
    assert moved.sum() > 200, f"{name}: {int(moved.sum())} pixels moved"
    assert (ref["color"] != other["color"]).any()
    if swap == SWAP_SHADOW_ON_IBL:
        assert not moved[ref["prequant"][..., 3] == 1].any()        # lit pixels keep their colour


# ---- the second restatement of the edge raster: float32 numpy -------------------------------------------------------

def _mat4_mul32(a, b):
    """glm's mat4 * mat4, column-major float32[16]: ((A0 b0 + A1 b1) + A2 b2) + A3 b3 per element"""
    a, b = np.asarray(a, F).reshape(4, 4), np.asarray(b, F).reshape(4, 4)   # [c][r]
    out = np.empty((4, 4), F)
    for c in range(4):
        for r in range(4):
            out[c, r] = F(F(F(a[0, r] * b[c, 0]) + F(a[1, r] * b[c, 1])) + F(a[2, r] * b[c, 2])) + F(a[3, r] * b[c, 3])
    return out.reshape(16)


def np_shadow_edge(size, light_vp, casters, tile, lanes):
    """draw_triangle_tile_shadow_xsimd (xsimd :1016-1191) and its tile jobs in float32 numpy: per triangle and job the box, then
    every texel of the box at once.  -> the map [h, w]"""
    w, h = (size, size) if isinstance(size, int) else size
    sm = np.full((h, w), FLT_MAX, F)
    jobs = [(tx * tile[0], ty * tile[1], min((tx + 1) * tile[0], w) - 1, min((ty + 1) * tile[1], h) - 1)
            for ty in range((h + tile[1] - 1) // tile[1]) for tx in range((w + tile[0] - 1) // tile[0])]
    with np.errstate(all="ignore"):
        for d in casters:
            lm = _mat4_mul32(light_vp, EYE if d.model is None else d.model)
            pos = np.asarray(d.mesh.positions, F).reshape(-1, 3)
            cx, cy, cz, cw = I._m4v(lm, pos)
            nx, ny, nz = (cx / cw).astype(F), (cy / cw).astype(F), (cz / cw).astype(F)
            sx = ((nx * F(0.5) + F(0.5)) * F(w - 1)).astype(F).reshape(-1, 3)
            sy = ((F(1) - (ny * F(0.5) + F(0.5))) * F(h - 1)).astype(F).reshape(-1, 3)
            sz, cw = nz.reshape(-1, 3), cw.reshape(-1, 3)
            for t in range(len(sx)):
                X, Y, Z = sx[t], sy[t], sz[t]
                if (np.abs(cw[t]) < F(1e-6)).any() or not (np.abs(X) < F(2147483648.0)).all() or not (np.abs(Y) < F(2147483648.0)).all():
                    continue
                area = F(F(X[1] - X[0]) * F(Y[2] - Y[0])) - F(F(Y[1] - Y[0]) * F(X[2] - X[0]))
                if np.abs(area) < F(1e-8) or area <= 0:
                    continue
                inv = F(1) / area
                fx0, cx1 = int(np.floor(X.min())), int(np.ceil(X.max()))
                fy0, cy1 = int(np.floor(Y.min())), int(np.ceil(Y.max()))
                A = [F(Y[0] - Y[1]), F(Y[1] - Y[2]), F(Y[2] - Y[0])]
                B = [F(X[1] - X[0]), F(X[2] - X[1]), F(X[0] - X[2])]
                C = [F(F(X[0] * Y[1]) - F(Y[0] * X[1])), F(F(X[1] * Y[2]) - F(Y[1] * X[2])), F(F(X[2] * Y[0]) - F(Y[2] * X[0]))]
                for (tminx, tminy, tmaxx, tmaxy) in jobs:
                    x0, x1 = min(max(max(tminx, fx0), 0), w - 1), min(max(min(tmaxx, cx1), 0), w - 1)
                    y0, y1 = min(max(max(tminy, fy0), 0), h - 1), min(max(min(tmaxy, cy1), 0), h - 1)
                    if x0 > x1 or y0 > y1:
                        continue
                    xs = np.arange(x0, x1 + 1)
                    body = (x0 + ((xs - x0) // lanes) * lanes + lanes - 1 <= x1)[None, :]
                    fx = (xs.astype(F) + F(0.5))[None, :]
                    fy = (np.arange(y0, y1 + 1).astype(F) + F(0.5))[:, None]
                    Ev = []
                    for k in range(3):
                        eb = (A[k] * fx).astype(F) + ((B[k] * fy).astype(F) + C[k]).astype(F)
                        et = ((A[k] * fx).astype(F) + (B[k] * fy).astype(F)).astype(F) + C[k]
                        Ev.append(np.where(body, eb, et).astype(F))
                    inside = (Ev[0] >= 0) & (Ev[1] >= 0) & (Ev[2] >= 0)
                    w0, w1, w2 = (Ev[1] * inv).astype(F), (Ev[2] * inv).astype(F), (Ev[0] * inv).astype(F)
                    z = (((w0 * Z[0]).astype(F) + (w1 * Z[1]).astype(F)).astype(F) + (w2 * Z[2]).astype(F)).astype(F)
                    ok = inside & (z >= 0) & (z <= 1)
                    view = sm[y0:y1 + 1, x0:x1 + 1]
                    view[ok & (z < view)] = z[ok & (z < view)]
    return sm


@pytest.mark.parametrize("name", list(EDGE_SCENES))
def test_edge_raster_equals_numpy_restatement(name):
    lvp, casters = EDGE_SCENES[name]()
    for size, tile, lanes in ((50, (160, 160), 8), (50, (16, 12), 4), ((33, 21), (7, 5), 16)):
        if name == "demo" and tile != (160, 160):
            continue                                    # (a thousand triangles: one job is enough for the witness)
        ref = ref_shadow_edge(size, lvp, casters, tile, lanes)
        got = np_shadow_edge(size, lvp, casters, tile, lanes)
        bad = np.argwhere(_bits(ref) != _bits(got))
        assert bad.size == 0, f"{name} {size} {tile} lanes {lanes}: {len(bad)} texels differ, first {bad[:4].tolist()}"


def test_edge_scenes_cover_what_the_gpu_tests_need():
    drawn = 0
    for name, fn in EDGE_SCENES.items():
        lvp, casters = fn()
        sm = ref_shadow_edge(50, lvp, casters)
        drawn += int((sm < FLT_MAX).any())
        assert ((sm == FLT_MAX) | ((sm >= 0) & (sm <= 1))).all(), name
    assert drawn >= 12


# ---- known answers of the edge raster -----------------------------------------------------------------------------

def test_mirror_image_is_dropped():
    lvp, casters = scene_mirror()
    sm = ref_shadow_edge(50, lvp, casters)
    assert (sm[:, :24] == F(0.5)).sum() > 100 and (sm[:, 24:] == FLT_MAX).all()      # the facing one writes, its mirror image nothing
    both = ref_shadow_edge(50, lvp, casters, swaps=SWAP_NO_CULL)
    assert (both[:, 24:] == F(0.25)).sum() > 100
    old = R.ref_shadow(50, lvp, casters, (160, 160))                                  # the barycentric raster draws both
    assert (old[:, 24:] < 1).sum() > 100 and (old[:, :24] < 1).sum() > 100


def test_triangle_left_of_the_map_visits_column_0_and_writes_nothing():
    lvp, casters = scene_left_of_map()
    for tile in EDGE_TILES:
        sm, vis = ref_shadow_edge(50, lvp, casters, tile, visits=True)
        assert (sm == FLT_MAX).all()
        assert vis[:, 0].sum() > 20 and not vis[:, 1:].any()
        assert not vis[:4, 0].any() and not vis[32:, 0].any()                         # rows 5 .. 30 only


# ---- rule swaps of the edge raster: each changes texels of a named scene ---------------------------------------------

EDGE_SWAPS = [(SWAP_BODY, "body association everywhere", "thirds"), (SWAP_TAIL, "tail association everywhere", "thirds"),
              (SWAP_STRICT, "strict > 0 edges", "thirds"), (SWAP_BC, "bc-style weights of the old raster", "random1"),
              (SWAP_NO_CULL, "no back-face drop", "windings"), (SWAP_NO_CEIL, "box without ceil", "random2")]


@pytest.mark.parametrize("swap,what,scene", EDGE_SWAPS, ids=[s[1].replace(" ", "-") for s in EDGE_SWAPS])
def test_edge_rule_swaps_change_texels(swap, what, scene):
    lvp, casters = EDGE_SCENES[scene]()
    ref = ref_shadow_edge(50, lvp, casters, (160, 160), 8)
    other = ref_shadow_edge(50, lvp, casters, (160, 160), 8, swaps=swap)
    n = int((_bits(ref) != _bits(other)).sum())
    assert n > 0, f"{what}: no texel of {scene} changed"
    # (the column and row that ceil adds lie beyond every corner, where an edge rejects the texel: what ceil changes is
    # max_x, so where the last whole lane group ends, so the association of a row's last texels)
    if swap in (SWAP_STRICT, SWAP_NO_CULL):
        assert ((ref == FLT_MAX) != (other == FLT_MAX)).any(), f"{what}: the covered set of {scene} did not change"


def test_lanes_4_8_16_give_three_maps_on_the_constructed_scene():
    """The association differs between a row's lane groups and its tail, and the grouping depends on the lane count: on
    scene_thirds (edges through texel centres, corners at thirds) the three maps differ pairwise, in depth bits and in which
    texels are covered at all."""
    lvp, casters = scene_thirds()
    maps = {l: ref_shadow_edge(50, lvp, casters, (160, 160), l) for l in (4, 8, 16)}
    for a, b in ((4, 8), (8, 16), (4, 16)):
        assert (_bits(maps[a]) != _bits(maps[b])).any(), f"lanes {a} and {b} give the same map"
    covered = {l: m < FLT_MAX for l, m in maps.items()}
    assert any((covered[a] != covered[b]).any() for a, b in ((4, 8), (8, 16), (4, 16)))
    # the tile job moves min_x and with it the grouping
    assert (_bits(ref_shadow_edge(50, lvp, casters, (7, 5), 8)) != _bits(maps[8])).any()
