"""tests/canvas_rt_pbr_ref (ref_canvas_rt_pbr.c), the C restatement of hello_pbr.cpp's camera pass, its GGX + IBL
fragment shader and the two IBL samplers -- the reference of tests/test_canvas_rt_pbr.py -- pinned on the CPU:

  * against a second restatement in float32 numpy, written from the same cited lines: fragment_shader_pbr and both
    samplers on seeded random samples and on every pixel of one small frame; everything before the final pow bit
    for bit (the sRGB table through libm's powf, as the C file takes it), the bytes under the parity rule of
    helpers.assert_color_parity (numpy's float32 power is another implementation);
  * by known answers of the samplers (ibl_known_cases, shared with the GPU test) and of the shader;
  * without a shadow map, an IBL or a changed normal matrix its raster is test_canvas_rt_ref's (depth, velocity,
    sub-triangles, texels, counters);
  * and the scenes of the GPU tests are checked to show, in the restatement's debug planes, what they are there for.

It also holds what fails without the feature and needs no GPU: the new entry points and the two new structs' sizes."""
import ctypes
import dataclasses
import functools
import os
import subprocess

import numpy as np

import helpers
import test_canvas_rt_ref as R
from test_canvas_rt_ref import F, H, SM, W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_pbr_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_pbr_ref.so")
_P = ctypes.c_void_p
DEN_CLAMPED = 1


class RefMaterial(ctypes.Structure):
    _fields_ = [("normal_mat", ctypes.c_float * 9), ("metallic", ctypes.c_float), ("roughness", ctypes.c_float), ("ao", ctypes.c_float),
                ("ibl_diffuse_intensity", ctypes.c_float), ("ibl_specular_intensity", ctypes.c_float),
                ("ibl_reflection_strength", ctypes.c_float)]


class RefConsts(ctypes.Structure):
    _fields_ = [("exposure", ctypes.c_float), ("min_roughness", ctypes.c_float), ("direct_intensity", ctypes.c_float)]


class RefIbl(ctypes.Structure):
    _fields_ = [("irr_size", ctypes.c_int32), ("irr", _P), ("spec_base", ctypes.c_int32), ("mip_count", ctypes.c_int32), ("spec", _P)]


class RefDebugPlanes(ctypes.Structure):
    _fields_ = [("face_n", _P), ("face_r", _P), ("m0", _P), ("m1", _P), ("pbr_flags", _P), ("prepow", _P), ("frag_in", _P), ("base", _P)]


@functools.lru_cache(maxsize=None)
def pbr_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    L.rcp_render.restype = ctypes.c_int
    L.rcp_render.argtypes = [ctypes.POINTER(R.RefFrame), ctypes.POINTER(RefConsts), ctypes.POINTER(RefIbl), ctypes.POINTER(R.RefDraw),
                             ctypes.POINTER(RefMaterial), ctypes.c_int, ctypes.POINTER(R.RefPlanes), ctypes.POINTER(RefDebugPlanes)]
    L.rcp_ibl_samples.restype = ctypes.c_int
    L.rcp_ibl_samples.argtypes = [ctypes.POINTER(RefIbl), ctypes.c_int] + [_P] * 5
    L.rcp_fragments.restype = ctypes.c_int
    L.rcp_fragments.argtypes = [ctypes.POINTER(R.RefFrame), ctypes.POINTER(RefConsts), ctypes.POINTER(RefIbl), ctypes.c_int, _P, _P, _P,
                                ctypes.POINTER(RefMaterial), _P, _P, _P, _P]
    return L


# ---- the IBL, the materials and the frames (shared with tests/test_canvas_rt_pbr.py) ------------------------

def make_ibl(seed=7, irr_size=4, spec_base=8, mips=4):
    """Seeded floats in [0, 4]: (irradiance [6, n, n, 3], [mip m: [6, s_m, s_m, 3]]) with s_m = max(1, spec_base >> m).
    The defaults have a size-1 level, clamped edges and the last-mip case."""
    rng = np.random.default_rng(seed)
    irr = rng.uniform(0.0, 4.0, (6, irr_size, irr_size, 3)).astype(F)
    spec = [rng.uniform(0.0, 4.0, (6, max(1, spec_base >> m), max(1, spec_base >> m), 3)).astype(F) for m in range(mips)]
    return irr, spec


def face_colour_ibl(irr_size=4, spec_base=8, mips=4):
    """Face f of every level is one constant colour (f + 1, 10 f + 0.5, 0.25 f)."""
    col = np.array([[f + 1.0, 10.0 * f + 0.5, 0.25 * f] for f in range(6)], F)
    lvl = lambda s: np.ascontiguousarray(np.broadcast_to(col[:, None, None, :], (6, s, s, 3)))   # noqa: E731
    return lvl(irr_size), [lvl(max(1, spec_base >> m)) for m in range(mips)], col


def _ibl_c(ibl, keep):
    if ibl is None:
        return None
    irr, spec = ibl
    irr = np.ascontiguousarray(irr, F)
    flat = np.concatenate([np.ascontiguousarray(m, F).reshape(-1) for m in spec])
    keep += [irr, flat]
    return RefIbl(irr.shape[1], irr.ctypes.data, spec[0].shape[1], len(spec), flat.ctypes.data)


def demo_consts(**kw):
    """shs_gpu.RtPbr with the demo's constants (hello_pbr.cpp:150-155), some replaced."""
    import shs_gpu
    return dataclasses.replace(shs_gpu.RtPbr(), **kw)


def _consts_c(k):
    k = demo_consts() if k is None else k
    return RefConsts(k.exposure, k.min_roughness, k.direct_intensity)


def material(normal_mat=None, **kw):
    import shs_gpu
    return shs_gpu.RtPbrDraw(normal_mat=None if normal_mat is None else np.asarray(normal_mat, F).reshape(9), **kw)


def normal_matrix(model):
    """transpose(inverse(mat3(model))) (:1557), column-major float32[9]: the caller's matrix, any values would do."""
    m3 = np.asarray(model, np.float64).reshape(4, 4).T[:3, :3]
    return np.ascontiguousarray(np.linalg.inv(m3), F).reshape(9)   # inv^T stored column-major is inv row by row


# The demo's three materials: floor plastic :1493-1504, car paint :1568-1579 (textured), golden monkey :1630-1641.
FLOOR = dict(color=(120, 122, 128, 255), metallic=0.0, roughness=0.70, ao=1.0, ibl_diffuse_intensity=1.30, ibl_specular_intensity=0.60,
             ibl_reflection_strength=0.20)
CAR = dict(color=(200, 200, 200, 255), metallic=0.0, roughness=0.22, ao=1.0, ibl_diffuse_intensity=1.50, ibl_specular_intensity=1.00,
           ibl_reflection_strength=1.20)
MONKEY = dict(color=(240, 195, 75, 255), metallic=0.95, roughness=0.20, ao=1.0, ibl_diffuse_intensity=1.00, ibl_specular_intensity=1.80,
              ibl_reflection_strength=1.00)
# The two materials of the edge-case scenes.  lod = roughness * 3 over the four mips: 1.0 gives m0 = m1 = 3 (the last
# mip), 0.35 gives m0 = 1; the demo's 0.70 and 0.20 / 0.22 give 2 and 0.  ao below 1 and intensities above 1 (saturated).
ROUGH_DIELECTRIC = dict(metallic=0.0, roughness=1.0, ao=0.8, ibl_diffuse_intensity=0.9, ibl_specular_intensity=0.7,
                        ibl_reflection_strength=2.0)
SMOOTH_METAL = dict(metallic=1.0, roughness=0.35, ao=1.0, ibl_diffuse_intensity=0.5, ibl_specular_intensity=1.0,
                    ibl_reflection_strength=0.75)
# Caller-supplied normal matrices (column-major) that turn the quads' (0, 0, -1) normals to the other faces' axes.
TO_PLUS_Z = (1, 0, 0, 0, 1, 0, 0, 0, -1)
TO_MINUS_Y = (1, 0, 0, 0, 0, 1, 0, 1, 0)
TO_PLUS_X = (0, 0, 1, 0, 1, 0, -1, 0, 0)
TO_MINUS_X = (0, 0, 1, 0, 1, 0, 1, 0, 0)
TO_PLUS_Y = (1, 0, 0, 0, 0, 1, 0, -1, 0)
TURNS = {"rough": [TO_PLUS_Z, TO_MINUS_Y, TO_PLUS_X], "metal": [None, TO_MINUS_X, TO_PLUS_Y]}


def with_material(draw, color=None, normal_mat=None, **mat):
    """(the RtDraw with the material's base colour, its RtPbrDraw)"""
    d = draw if color is None else dataclasses.replace(draw, base_color=color)
    return d, material(normal_mat, **mat)


def demo_scene(light_kw=None, monkey_color=None):
    """test_canvas_rt_ref.scene_demo with the demo's three materials: the floor (normal_mat = mat3(1)), the monkey,
    the textured quad as the car."""
    view, lvp, draws = R.scene_demo(light_kw)
    mk = dict(MONKEY) if monkey_color is None else dict(MONKEY, color=monkey_color)
    pairs = [with_material(draws[0], **FLOOR), with_material(draws[1], normal_mat=normal_matrix(draws[1].model), **mk),
             with_material(draws[2], normal_mat=normal_matrix(draws[2].model), **CAR)]
    return view, lvp, [p[0] for p in pairs], [p[1] for p in pairs]


def edge_scene(name, which):
    """R.SCENES[name] under one of the two edge-case materials, the normals turned by TURNS[which]."""
    view, lvp, draws = R.SCENES[name]()
    mat = ROUGH_DIELECTRIC if which == "rough" else SMOOTH_METAL
    turns = TURNS[which]
    mats = [material(turns[i % 3], **mat) for i in range(len(draws))]
    return view, lvp, draws, mats


def pbr_frame(view, light_vp, w=W, h=H, tile=(80, 80), **kw):
    return R._frame(view, light_vp, w, h, tile, shading=2, **kw)


def _frame_c(frame, shadow, keep):
    f = R.RefFrame()
    f.W, f.H = frame.width, frame.height
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
        keep.append(sm)
        f.shadow, f.sw, f.sh = sm.ctypes.data, sm.shape[1], sm.shape[0]
    return f


def _materials_c(mats):
    arr = (RefMaterial * max(len(mats), 1))()
    for i, m in enumerate(mats):
        n3 = np.eye(3, dtype=F).reshape(9) if m.normal_mat is None else np.asarray(m.normal_mat, F).reshape(9)
        arr[i].normal_mat[:] = [float(v) for v in n3]
        for name in ("metallic", "roughness", "ao", "ibl_diffuse_intensity", "ibl_specular_intensity", "ibl_reflection_strength"):
            setattr(arr[i], name, float(getattr(m, name)))
    return arr


def ref_render_pbr(frame, draws, mats, shadow=None, ibl=None, consts=None):
    """The PBR PASS1 of a shs_gpu.RtFrame -> test_canvas_rt_ref.ref_render's planes and counters, plus the debug planes
    'face_n', 'face_r', 'm0', 'm1', 'pbr_flags', 'prepow' [.., 3], 'frag_in' [.., 6] and 'base' [.., 3] (canvas rows)."""
    Wd, Hd = frame.width, frame.height
    keep = []
    arr = R._ref_draws(draws, keep)
    f = _frame_c(frame, shadow, keep)
    out = {"color": np.empty((Hd, Wd, 4), np.uint8), "depth": np.empty((Hd, Wd), F), "velocity": np.empty((Hd, Wd, 2), F),
           "prequant": np.empty((Hd, Wd, 4), F), "tri_id": np.empty((Hd, Wd), np.int32), "texel": np.empty((Hd, Wd), np.int32),
           "flags": np.empty((Hd, Wd), np.int32)}
    dbg = {k: np.empty((Hd, Wd), np.int32) for k in ("face_n", "face_r", "m0", "m1", "pbr_flags")}
    dbg.update(prepow=np.empty((Hd, Wd, 3), F), frag_in=np.empty((Hd, Wd, 6), F), base=np.empty((Hd, Wd, 3), np.uint8))
    p, g = R.RefPlanes(), RefDebugPlanes()
    for k, v in out.items():
        setattr(p, k, v.ctypes.data)
    for k, v in dbg.items():
        setattr(g, k, v.ctypes.data)
    kc, ic = _consts_c(consts), _ibl_c(ibl, keep)
    assert pbr_lib().rcp_render(ctypes.byref(f), ctypes.byref(kc), None if ic is None else ctypes.byref(ic), arr, _materials_c(mats),
                                len(draws), ctypes.byref(p), ctypes.byref(g)) == 0
    out.update(dbg)
    out["counters"] = dict(zip(("input_tris", "polys3", "polys4", "sub_tris"), (int(c) for c in p.counters)))
    return out


def ref_ibl_samples(ibl, dirs, lod):
    """-> (irradiance [n, 3], specular [n, 3], debug [n, 4]: irradiance face, specular face, m0, m1)"""
    keep = []
    ic = _ibl_c(ibl, keep)
    dirs = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    n = dirs.shape[0]
    lod = np.ascontiguousarray(lod, F).reshape(n)
    a, b, d = np.empty((n, 3), F), np.empty((n, 3), F), np.empty((n, 4), np.int32)
    assert pbr_lib().rcp_ibl_samples(ctypes.byref(ic), n, dirs.ctypes.data, lod.ctypes.data, a.ctypes.data, b.ctypes.data, d.ctypes.data) == 0
    return a, b, d


def ref_fragments(frame, normal, world, base, mats, shadow=None, ibl=None, consts=None):
    """fragment_shader_pbr of n fragments -> (pre [n, 4], prepow [n, 3], rgba [n, 4], debug [n, 5])"""
    keep = []
    f = _frame_c(frame, shadow, keep)
    normal, world = np.ascontiguousarray(normal, F).reshape(-1, 3), np.ascontiguousarray(world, F).reshape(-1, 3)
    n = normal.shape[0]
    base = np.ascontiguousarray(base, np.uint8).reshape(n, 3)
    pre, prepow, rgba, dbg = np.empty((n, 4), F), np.empty((n, 3), F), np.empty((n, 4), np.uint8), np.empty((n, 5), np.int32)
    kc, ic = _consts_c(consts), _ibl_c(ibl, keep)
    assert pbr_lib().rcp_fragments(ctypes.byref(f), ctypes.byref(kc), None if ic is None else ctypes.byref(ic), n, normal.ctypes.data,
                                   world.ctypes.data, base.ctypes.data, _materials_c(mats), pre.ctypes.data, prepow.ctypes.data,
                                   rgba.ctypes.data, dbg.ctypes.data) == 0
    return pre, prepow, rgba, dbg


# ---- sample sets and known answers of the samplers (shared with the GPU test) ---------------------------------

def random_directions(seed=21, n=4096, mips=4):
    """n directions of every length and sign, some along axes and diagonals, with lods from below 0 to above mips - 1."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)).astype(F) * rng.choice(np.array([1e-3, 1.0, 50.0], F), size=(n, 1))
    d[::64] = np.sign(d[::64]) * F(0.75)                       # |x| == |y| == |z|: the tie order decides
    d[1::64, 1] = d[1::64, 0]                                  # |x| == |y|
    d[2::64, 2] = -d[2::64, 1]                                 # |y| == |z|
    lod = rng.uniform(-0.5, mips - 0.5, n).astype(F)
    lod[::16] = rng.integers(0, mips, len(lod[::16])).astype(F)   # exactly on a mip
    return d, lod


def ibl_known_cases():
    """(name, direction, lod, irradiance face or None for 0, m0, m1) over face_colour_ibl(): a constant face returns its
    colour whatever the bilinear weights, and mix(c, c, t) of one face's colour is that colour at any lod."""
    axes = [("+x", (1, 0, 0), 0), ("-x", (-1, 0, 0), 1), ("+y", (0, 1, 0), 2), ("-y", (0, -1, 0), 3), ("+z", (0, 0, 1), 4),
            ("-z", (0, 0, -1), 5)]
    cases = [(n, d, lod, f, min(int(lod), 3), min(int(lod) + 1, 3)) for n, d, f in axes for lod in (0.0, 0.5, 1.25, 2.75, 3.0)]
    cases += [
        ("zero", (0, 0, 0), 1.5, None, 1, 2),
        ("tiny", (1e-9, -1e-9, 1e-9), 1.5, None, 1, 2),          # length below 1e-8
        ("tie-xyz+", (2, 2, 2), 0.0, 0, 0, 1),                   # ax >= ay && ax >= az comes first
        ("tie-xyz-", (-2, -2, -2), 0.0, 1, 0, 1),
        ("tie-yz", (1, 3, -3), 0.0, 2, 0, 1),                    # ay >= ax && ay >= az before z
        ("tie-xz", (-3, 1, 3), 0.0, 1, 0, 1),
        ("tie-xy", (3, -3, 1), 0.0, 0, 0, 1),
        ("lod-below", (0, 0, 5), -2.0, 4, 0, 1),                 # clamps to 0
        ("lod-above", (0, 0, 5), 7.5, 4, 3, 3),                  # clamps to mip_count - 1, m1 == m0
        ("lod-last", (0, -5, 0), 3.0, 3, 3, 3),
    ]
    return cases


def edge_directions():
    """Zero-length and NaN directions and lods.  IEEE 754 leaves a NaN's sign and payload to the implementation, and either
    compiler may commute the operands that decide them, so results are compared with every NaN made one NaN
    (canonical_bits): where a value is a number its bits must be equal, where it is a NaN both must be NaNs."""
    nan = float("nan")
    d = np.array([(0, 0, 0), (-0.0, 0.0, -0.0), (1e-9, 0, 0), (nan, 0, 0), (0, nan, 1), (1, 2, nan), (nan, nan, nan), (1, 0, 0),
                  (0, 3, 0), (1, 1, 1)], F)
    lod = np.array([0.5, 1.0, 2.0, 0.5, 1.5, 2.5, 0.0, nan, -1.0, 9.0], F)
    return d, lod


def canonical_bits(a):
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


# ---- what fails without the feature, without a GPU ---------------------------------------------------------

NEW_ENTRY_POINTS = ("shs_rt_set_pbr", "shs_rt_set_ibl", "shs_rt_render_pbr", "shs_rt_ibl_samples")


def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in NEW_ENTRY_POINTS + ("shs_rt_render",):
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_ctypes_pbr_structs_have_the_headers_sizes(tmp_path):
    from shs_gpu import _abi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(shs_rt_pbr_draw), '
                   'sizeof(shs_rt_pbr), sizeof(shs_rt_frame), sizeof(shs_rt_draw)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_abi.RtPbrDrawC), ctypes.sizeof(_abi.RtPbrC), ctypes.sizeof(_abi.RtFrameC), ctypes.sizeof(_abi.RtDrawC)]
    assert sizes[:2] == [60, 12] and sizes[:2] == [ctypes.sizeof(RefMaterial), ctypes.sizeof(RefConsts)]


# ---- the second restatement: float32 numpy -----------------------------------------------------------------

def _powf_table():
    """srgb_to_linear of the 256 bytes with libm's powf, the function the C restatement calls."""
    libm = ctypes.CDLL("libm.so.6")
    libm.powf.restype = ctypes.c_float
    libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
    return np.array([libm.powf(float(F(c) / F(255)), 2.2) for c in range(256)], F)


def _sat(x):
    return np.where(x < F(0), F(0), np.where(x > F(1), F(1), x)).astype(F)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    return v * (F(1) / np.sqrt(_dot(v, v)))[..., None]


def np_cube(level, d):
    """sample_cubemap_linear_vec (ibl.hpp:236-270) of level [6, s, s, 3] at directions d [n, 3] -> ([n, 3], face [n])."""
    level, d = np.asarray(level, F), np.asarray(d, F)
    s = level.shape[1]
    ln = np.sqrt(_dot(d, d))
    zero = ln < F(1e-8)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = d / ln[:, None]
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        cx = (ax >= ay) & (ax >= az)
        cy = ~cx & (ay >= ax) & (ay >= az)
        face = np.where(cx, np.where(x > 0, 0, 1), np.where(cy, np.where(y > 0, 2, 3), np.where(z > 0, 4, 5)))
        u = np.choose(face, [-z / ax, z / ax, x / ay, x / ay, x / az, -x / az])
        v = np.choose(face, [y / ax, y / ax, -z / ay, z / ay, y / az, y / az])
    u, v = F(0.5) * (u + F(1)), F(0.5) * (v + F(1))
    u, v = np.where(zero, F(0), u), np.where(zero, F(0), v)
    u = np.where(u < 0, F(0), np.where(u > 1, F(1), u)).astype(F)
    v = np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)
    fx, fy = u * F(s - 1), v * F(s - 1)
    x0 = np.clip(np.floor(fx).astype(np.int64), 0, s - 1)
    y0 = np.clip(np.floor(fy).astype(np.int64), 0, s - 1)
    x1, y1 = np.clip(x0 + 1, 0, s - 1), np.clip(y0 + 1, 0, s - 1)
    tx, ty = (fx - x0.astype(F))[:, None], (fy - y0.astype(F))[:, None]
    mix = lambda a, b, t: a * (F(1) - t) + b * t   # noqa: E731
    c0 = mix(level[face, y0, x0], level[face, y0, x1], tx)
    c1 = mix(level[face, y1, x0], level[face, y1, x1], tx)
    out = mix(c0, c1, ty)
    out[zero] = 0
    return out.astype(F), np.where(zero, -1, face)


def np_trilinear(spec, d, lod):
    """sample_prefiltered_spec_trilinear (ibl.hpp:272-286) -> ([n, 3], m0, m1)"""
    mips = len(spec)
    lod = np.asarray(lod, F)
    lod = np.where(lod < 0, F(0), np.where(lod > F(mips - 1), F(mips - 1), lod)).astype(F)
    m0 = np.floor(lod).astype(np.int64)
    m1 = np.minimum(m0 + 1, mips - 1)
    t = (lod - m0.astype(F))[:, None]
    per = [np_cube(m, d)[0] for m in spec]
    c0 = np.stack(per)[m0, np.arange(len(lod))]
    c1 = np.stack(per)[m1, np.arange(len(lod))]
    return (c0 * (F(1) - t) + c1 * t).astype(F), m0, m1


def np_fragments(frame, normal, world, base, mats, shadow, ibl, consts):
    """fragment_shader_pbr (hello_pbr.cpp:627-727) in float32 numpy over n fragments; shadow [n]: the factor the shadow
    lookup gave (that lookup is the hard demo's, pinned by test_canvas_rt_ref).  mats: a dict of [n] arrays.
    -> (prepow [n, 3], pre [n, 3])"""
    k = demo_consts() if consts is None else consts
    N = _normalize(np.asarray(normal, F))
    V = _normalize(np.asarray(frame.camera_pos, F)[None, :] - np.asarray(world, F))
    L = _normalize(-np.asarray(frame.light_dir_world, F))[None, :]
    Hh = _normalize(V + L)
    zero = F(0)
    mx0 = lambda x: np.where(zero < x, x, zero).astype(F)   # noqa: E731  glm::max(0, x)
    NoV, NoL, NoH = mx0(_dot(N, V)), mx0(_dot(N, np.broadcast_to(L, N.shape))), mx0(_dot(N, Hh))
    lin = _powf_table()[np.asarray(base, np.uint8)]
    metallic = _sat(mats["metallic"])
    r = mats["roughness"].astype(F)
    roughness = np.where(r < F(k.min_roughness), F(k.min_roughness), np.where(r > F(1), F(1), r)).astype(F)
    ao = _sat(mats["ao"])
    om = F(1) - metallic
    F0 = F(0.04) * om[:, None] + lin * metallic[:, None]
    x = F(1) - _sat(NoV)
    x2 = x * x
    x5 = (x2 * x2 * x)[:, None]
    Fr = (F0 + (F(1) - F0) * x5) * np.array([1.0, 0.96, 0.90], F)[None, :]
    kd = (F(1) - Fr) * om[:, None]
    PI = F(3.14159265358979323846)
    a2 = (roughness * roughness) * (roughness * roughness)
    nh = _sat(NoH)
    dd = (nh * nh) * (a2 - F(1)) + F(1)
    D = a2 / (PI * dd * dd)
    r1 = roughness + F(1)
    kk = (r1 * r1) / F(8)
    gs = lambda c: _sat(c) / (_sat(c) * (F(1) - kk) + kk)   # noqa: E731
    G = gs(NoV) * gs(NoL)
    den = np.where(F(1e-6) < F(4) * NoV * NoL, F(4) * NoV * NoL, F(1e-6)).astype(F)
    direct = (kd * lin * (F(1) / PI) + ((D * G)[:, None] * Fr) / den[:, None]) * F(k.direct_intensity) * NoL[:, None]
    direct = direct * np.asarray(shadow, F)[:, None]
    amb = np.zeros_like(direct)
    if ibl is not None:
        irr, spec = ibl
        diff = np_cube(irr, N)[0] * lin * kd * _sat(mats["ibl_diffuse_intensity"])[:, None]
        I = -V
        R_ = I - N * _dot(N, I)[:, None] * F(2)
        pre = np_trilinear(spec, R_, roughness * F(len(spec) - 1))[0]
        ss = _sat(mats["ibl_specular_intensity"]) * _sat(mats["ibl_reflection_strength"])
        amb = diff + pre * Fr * ss[:, None]
    c = direct + amb * ao[:, None]
    c = c + lin * F(0.03) * ao[:, None]
    c = c * F(k.exposure)
    c = c / (F(1) + c)
    prepow = np.minimum(np.maximum(c, F(0)), F(1)).astype(F)
    srgb = np.power(prepow, F(1.0) / F(2.2)).astype(F)
    return prepow, (np.minimum(np.maximum(srgb, F(0)), F(1)) * F(255)).astype(F)


def _mats_arrays(mats, who=None):
    names = ("metallic", "roughness", "ao", "ibl_diffuse_intensity", "ibl_specular_intensity", "ibl_reflection_strength")
    pick = range(len(mats)) if who is None else who
    return {n: np.array([getattr(mats[i], n) for i in pick], F) for n in names}


def _assert_second_restatement(frame, normal, world, base, mats_list, mats_arr, shadow_map, ibl, consts):
    pre, prepow, rgba, _ = ref_fragments(frame, normal, world, base, mats_list, shadow_map, ibl, consts)
    np_prepow, np_pre = np_fragments(frame, normal, world, base, mats_arr, pre[:, 3], ibl, consts)
    bad = np.argwhere(np_prepow.view(np.uint32) != prepow.view(np.uint32))
    assert bad.size == 0, f"{len(bad)} of {prepow.size} channels differ before the pow, first {bad[:4].tolist()}"
    np_rgba = np.concatenate([np_pre.astype(np.uint8), np.full((len(pre), 1), 255, np.uint8)], axis=1)
    helpers.assert_color_parity(np_rgba[None], rgba[None], np_pre[None], pre[None, :, :3])


def random_fragments(seed=31, n=3000):
    """Normals of any length, world positions around the scene, random bytes and materials beyond [0, 1]."""
    import shs_gpu
    rng = np.random.default_rng(seed)
    normal = rng.normal(size=(n, 3)).astype(F) * rng.uniform(0.2, 3.0, (n, 1)).astype(F)
    world = rng.uniform([-8, -1, -4], [8, 6, 12], (n, 3)).astype(F)
    base = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    vals = rng.uniform(-0.2, 1.3, (n, 6)).astype(F)
    vals[:, 3:] = rng.uniform(-0.2, 2.0, (n, 3)).astype(F)
    mats = [shs_gpu.RtPbrDraw(None, *[float(v) for v in row]) for row in vals]
    return normal, world, base, mats


def test_numpy_restatement_on_random_fragments():
    view, lvp, draws, _ = demo_scene()
    shadow = R.ref_shadow(SM, lvp, draws)
    normal, world, base, mats = random_fragments()
    for ibl, consts, use_shadow in ((make_ibl(), None, True), (None, None, False),
                                    (make_ibl(3, 5, 6, 3), demo_consts(exposure=0.9, min_roughness=0.1, direct_intensity=5.0), True)):
        frame = pbr_frame(view, lvp, use_shadow=use_shadow)
        _assert_second_restatement(frame, normal, world, base, mats, _mats_arrays(mats), shadow if use_shadow else None, ibl, consts)


def test_numpy_restatement_on_every_pixel_of_a_small_frame():
    w, h = 33, 31
    view, proj = R.camera(w, h)
    _, lvp, draws, mats = demo_scene()
    draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
    shadow = R.ref_shadow(50, lvp, draws)
    frame = pbr_frame(view, lvp, w, h)
    ibl = make_ibl()
    ref = ref_render_pbr(frame, draws, mats, shadow, ibl)
    px = ref["tri_id"] >= 0
    assert px.sum() > 500
    ends = np.cumsum([d.mesh.positions.shape[0] for d in draws])
    who = np.searchsorted(ends, ref["tri_id"][px] // 2, side="right")
    assert set(who.tolist()) == {0, 1, 2}
    fi = ref["frag_in"][px]
    prepow, pre = np_fragments(frame, fi[:, :3], fi[:, 3:], ref["base"][px], _mats_arrays(mats, who), ref["prequant"][px][:, 3], ibl, None)
    assert np.array_equal(prepow.view(np.uint32), ref["prepow"][px].view(np.uint32))
    rgba = np.concatenate([pre.astype(np.uint8), np.full((len(pre), 1), 255, np.uint8)], axis=1)
    helpers.assert_color_parity(rgba[None], ref["color"][px][None], pre[None], ref["prequant"][px][None, :, :3])


def test_numpy_samplers_equal_the_restatement_bitwise():
    for ibl in (make_ibl(), make_ibl(5, 1, 1, 1), make_ibl(9, 3, 5, 6)):
        d, lod = random_directions(mips=len(ibl[1]))
        a, b, dbg = ref_ibl_samples(ibl, d, lod)
        na, nf = np_cube(ibl[0], d)
        nb, m0, m1 = np_trilinear(ibl[1], d, lod)
        assert np.array_equal(na.view(np.uint32), a.view(np.uint32)) and np.array_equal(nf, dbg[:, 0])
        assert np.array_equal(nb.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(m0, dbg[:, 2]) and np.array_equal(m1, dbg[:, 3])
        assert set(dbg[:, 0].tolist()) == set(range(6)) and set(dbg[:, 2].tolist()) == set(range(len(ibl[1])))


# ---- known answers ------------------------------------------------------------------------------------------

def test_sampler_known_answers():
    irr, spec, col = face_colour_ibl()
    for name, d, lod, face, m0, m1 in ibl_known_cases():
        a, b, dbg = ref_ibl_samples((irr, spec), [d], [lod])
        want = np.zeros(3, F) if face is None else col[face]
        assert np.array_equal(a[0], want) and np.array_equal(b[0], want), (name, a[0], b[0])
        assert (dbg[0, 0], dbg[0, 1]) == ((-1, -1) if face is None else (face, face)), (name, dbg[0])
        assert (dbg[0, 2], dbg[0, 3]) == (m0, m1), (name, dbg[0])


def test_sampler_edge_directions_stay_in_bounds():
    """NaN coordinates convert to INT_MIN and are clamped to texel 0 / 1; a NaN lod to mip 0.  Every output is 0 (zero
    length), a NaN (a NaN coordinate weights the texels) or a value of the maps' range."""
    ibl = make_ibl()
    d, lod = edge_directions()
    a, b, dbg = ref_ibl_samples(ibl, d, lod)
    assert (a[:3] == 0).all() and (b[:3] == 0).all() and (dbg[:3, :2] == -1).all()
    assert np.isnan(a[3:7]).all() and np.isnan(b[3:7]).all()
    assert np.isfinite(a[7:]).all() and np.isnan(b[7]).all() and np.isfinite(b[8:]).all()   # (b[7]: the NaN lod weights the mips)
    assert (dbg[7, 2], dbg[7, 3]) == (0, 1) and (dbg[8, 2], dbg[9, 2], dbg[9, 3]) == (0, 3, 3)


def _one(frame, n, wp, base, mat, shadow=None, ibl=None, consts=None):
    pre, prepow, rgba, dbg = ref_fragments(frame, [n], [wp], [base], [mat], shadow, ibl, consts)
    return pre[0], prepow[0], dbg[0]


def _encode(lin, consts=None):
    """exposure, Reinhard and the clamp of a linear colour, as the shader ends"""
    k = demo_consts() if consts is None else consts
    c = np.asarray(lin, F) * F(k.exposure)
    c = c / (F(1) + c)
    return np.minimum(np.maximum(c, F(0)), F(1)).astype(F)


def test_shader_known_answers():
    view, lvp, _, _ = demo_scene()
    lut = _powf_table()
    frame = pbr_frame(view, lvp, use_shadow=False)
    Ld = np.asarray(R.LIGHT_DIR, np.float64)
    to_light = tuple(-Ld / np.linalg.norm(Ld))
    wp, base = (0.5, 1.0, 2.0), (200, 120, 40)
    lin = lut[list(base)]
    ibl = make_ibl()
    # NoL = 0 (the normal points away from the light): direct is exactly 0, so without an IBL the colour is the minimum
    # ambient base * 0.03 * ao alone, and the max(1e-6, 4 NoV NoL) clamp is taken
    away = tuple(-v for v in to_light)
    m = material(metallic=0.3, roughness=0.5, ao=0.6)
    pre, prepow, dbg = _one(frame, away, wp, base, m)
    assert np.array_equal(prepow, _encode(lin * F(0.03) * F(0.6))) and dbg[4] & DEN_CLAMPED and tuple(dbg[:4]) == (-1, -1, -1, -1)
    # ao = 0 leaves direct alone: the same fragment with and without the IBL, lit
    m0 = material(metallic=0.3, roughness=0.5, ao=0.0)
    lit = (0.2, 0.9, -0.4)
    a = _one(frame, lit, wp, base, m0, ibl=ibl)
    b = _one(frame, lit, wp, base, m0)
    assert np.array_equal(a[1], b[1]) and (a[1] > 0).all() and not a[2][4] & DEN_CLAMPED
    # metallic = 1 makes kd zero: the diffuse terms vanish, so neither the irradiance map nor the diffuse intensity matters
    mm = material(metallic=1.0, roughness=0.4, ao=1.0, ibl_diffuse_intensity=1.0)
    mm2 = dataclasses.replace(mm, ibl_diffuse_intensity=0.0)
    ibl2 = (ibl[0] * F(3), ibl[1])
    ra, rb, rc = _one(frame, lit, wp, base, mm, ibl=ibl), _one(frame, lit, wp, base, mm2, ibl=ibl), _one(frame, lit, wp, base, mm, ibl=ibl2)
    assert np.array_equal(ra[1], rb[1]) and np.array_equal(ra[1], rc[1])
    md = dataclasses.replace(mm, metallic=0.0)
    assert not np.array_equal(_one(frame, lit, wp, base, md, ibl=ibl)[1], _one(frame, lit, wp, base, md, ibl=ibl2)[1])
    # a shadow factor of 0 leaves IBL + minimum ambient: a map of zeros under an identity light_vp shadows z = 0.5, and
    # the fragment equals the unshadowed one under a light of intensity 0
    eye = np.eye(4, dtype=F).reshape(16)
    fs = pbr_frame(view, eye, use_shadow=True)
    p5 = (0.1, 0.2, 0.5)
    sh = _one(fs, lit, p5, base, md, shadow=np.zeros((2, 2), F), ibl=ibl)
    dark = _one(frame, lit, p5, base, md, ibl=ibl, consts=demo_consts(direct_intensity=0.0))
    assert sh[0][3] == 0.0 and _one(fs, lit, p5, base, md, shadow=np.ones((2, 2), F), ibl=ibl)[0][3] == 1.0
    assert np.array_equal(sh[1], dark[1]) and (sh[1] < _one(frame, lit, p5, base, md, ibl=ibl)[1]).all()
    # no IBL leaves direct + base * 0.03 * ao: the same as an IBL whose two intensities are 0, and removing the minimum
    # ambient (ao = 0) lowers every channel
    m1 = material(metallic=0.3, roughness=0.5, ao=1.0, ibl_diffuse_intensity=0.0, ibl_specular_intensity=0.0)
    with_amb = _one(frame, lit, wp, base, m1)
    assert np.array_equal(with_amb[1], _one(frame, lit, wp, base, m1, ibl=ibl)[1]) and (with_amb[1] > b[1]).all()
    # the sRGB table: entry 0 is 0, entry 255 is 1, monotone
    assert lut[0] == 0 and lut[255] == 1 and (np.diff(lut) > 0).all()


def test_raster_is_the_hard_demos_without_the_shader():
    """Depth, velocity, sub-triangles, texels and counters of the PBR pass equal test_canvas_rt_ref's pass, whatever the
    normal matrices and the IBL: the two rasters differ in the fragment shader alone."""
    view, lvp, draws, mats = demo_scene()
    shadow = R.ref_shadow(SM, lvp, draws)
    hard = R.ref_render(R._frame(view, lvp), draws, shadow)
    pbr = ref_render_pbr(pbr_frame(view, lvp), draws, mats, shadow, make_ibl())
    for k in ("depth", "velocity", "tri_id", "texel"):
        assert np.array_equal(hard[k].view(np.uint8), pbr[k].view(np.uint8)), k
    assert hard["counters"] == pbr["counters"]


# ---- what the GPU scenes are there for -------------------------------------------------------------------

# What tests/test_canvas_rt_pbr.py's frames must exercise, counted on the restatement alone over (a) the demo in
# miniature with PCF and (b) the eight edge scenes, all under make_ibl(); (c) the no-IBL demo frame whose monkey has
# a zero blue byte; (d) the demo frame under SATURATING.  The counts this file's author measured are in the comments;
# each bound leaves room to spare.
SATURATING = dict(direct_intensity=1e9)   # 4e7 after the exposure: x / (1 + x) rounds to 1 on lit pixels
NEED = {
    "shadow factor 0": 300,              # 4,120
    "shadow factor between": 50,         # 15,849
    "shadow factor 1": 3000,             # 64,245
    "pixels per face of N (min)": 40,    # 1,710 (-y)
    "pixels per face of R (min)": 40,    # 372 (-y)
    "values of m0": 4,                   # 0, 1, 2, 3
    "m1 == m0 at the last mip": 1000,    # 20,984
    "textured pixels": 300,              # 8,542
    "untextured pixels": 3000,           # 75,672
    "metallic below 0.05": 3000,         # 61,259
    "metallic above 0.9": 3000,          # 22,955
    "channels at 255": 1000,             # 37,772
    "channels at 0": 100,                # 289
    "den clamped": 300,                  # 10,077
    "den not clamped": 3000,             # 74,137
}


def _count_scenes():
    ibl = make_ibl()
    got = dict.fromkeys(NEED, 0)
    faces_n, faces_r, m0s = np.zeros(6, np.int64), np.zeros(6, np.int64), set()
    frames = []
    view, lvp, draws, mats = demo_scene()
    frames.append((view, lvp, draws, mats, ibl, None))
    for name in ("windings", "near", "coincident", "outside"):
        for which in ("rough", "metal"):
            frames.append(edge_scene(name, which) + (ibl, None))
    view, lvp, draws0, mats0 = demo_scene(monkey_color=(240, 195, 0, 255))
    frames.append((view, lvp, draws0, mats0, None, None))
    frames.append((view, lvp, draws, mats, ibl, demo_consts(**SATURATING)))
    for view, lvp, dr, ms, ib, consts in frames:
        shadow = R.ref_shadow(SM, lvp, dr)
        ref = ref_render_pbr(pbr_frame(view, lvp), dr, ms, shadow, ib, consts)
        px = ref["tri_id"] >= 0
        s = ref["prequant"][..., 3][px]
        got["shadow factor 0"] += int((s == 0).sum())
        got["shadow factor between"] += int(((s > 0) & (s < 1)).sum())
        got["shadow factor 1"] += int((s == 1).sum())
        if ib is not None:
            faces_n += np.bincount(ref["face_n"][px], minlength=6)
            faces_r += np.bincount(ref["face_r"][px], minlength=6)
            m0s |= set(ref["m0"][px].tolist())
            got["m1 == m0 at the last mip"] += int(((ref["m0"][px] == 3) & (ref["m1"][px] == 3)).sum())
        got["textured pixels"] += int((ref["texel"][px] >= 0).sum())
        got["untextured pixels"] += int((ref["texel"][px] < 0).sum())
        ends = np.cumsum([d.mesh.positions.shape[0] for d in dr])
        met = np.array([m.metallic for m in ms], F)[np.searchsorted(ends, ref["tri_id"][px] // 2, side="right")]
        got["metallic below 0.05"] += int((met < 0.05).sum())
        got["metallic above 0.9"] += int((met > 0.9).sum())
        got["channels at 255"] += int((ref["color"][px][:, :3] == 255).sum())
        got["channels at 0"] += int((ref["color"][px][:, :3] == 0).sum())
        clamped = (ref["pbr_flags"][px] & DEN_CLAMPED) != 0
        got["den clamped"] += int(clamped.sum())
        got["den not clamped"] += int((~clamped).sum())
    got["pixels per face of N (min)"] = int(faces_n.min())
    got["pixels per face of R (min)"] = int(faces_r.min())
    got["values of m0"] = len(m0s)
    return got, faces_n, faces_r


def test_scenes_cover_what_the_gpu_tests_need():
    got, faces_n, faces_r = _count_scenes()
    short = {k: (got[k], NEED[k]) for k in NEED if got[k] < NEED[k]}
    assert not short, f"{short} (faces of N {faces_n.tolist()}, of R {faces_r.tolist()})"
