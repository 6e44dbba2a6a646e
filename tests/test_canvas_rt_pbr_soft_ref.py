"""tests/canvas_rt_pbr_soft_ref (ref_canvas_rt_pbr_soft.c), the C restatement of hello_pbr_light_shafts.cpp's camera pass
(PASS1: hello_pbr.cpp's raster, its fragment_shader_pbr :768-850 under pcss_shadow_factor :650-762) -- the reference of
tests/test_canvas_rt_pbr_soft.py -- pinned on the CPU:

  * cross-pin 1: without a shadow map and with every ao = 0 its frame is test_canvas_rt_pbr_ref's (shading 2), byte for
    byte and float for float -- the raster and everything of the shader but the shadow factor and the minimum ambient;
  * cross-pin 2: with a map, the (uv, z, bias, px, py) it hands to its PCSS give, through test_canvas_rt_soft_ref's
    rcs_pcss_samples (another text of the same function, over a clamping map), its factor plane bit for bit;
  * known answers for the three differences from shading 2;
  * a second restatement in float32 numpy (np_fragments_soft, whose PCSS is test_canvas_rt_soft_ref.np_pcss), bit for bit
    up to the final powf, on random fragments and on every pixel of a 40 x 30 frame;
  * and the frames of the GPU tests are checked to show, in the restatement's debug planes, what they are there for.

It also holds what fails without the feature and needs no GPU: the new entry point."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
import test_canvas_rt_soft_ref as S
from test_canvas_rt_ref import F, FLT_MAX, H, SM, W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_pbr_soft_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_pbr_soft_ref.so")
_P = ctypes.c_void_p
UV_OUTSIDE, EMPTY_CENTRE, NO_BLOCKER, BLOCKER_OFF_MAP, BLOCKER_EMPTY, PCF_OFF_MAP, PCF_EMPTY, NOT_IN_LIGHT = 1, 2, 4, 8, 16, 32, 64, 128
RADIUS_AT_MIN, RADIUS_AT_MAX = 256, 512
EDGE_NAMES = ("windings", "near", "coincident", "outside")


class RefPcssPlanes(ctypes.Structure):
    _fields_ = [("blockers", _P), ("radius", _P), ("pcss_flags", _P), ("pcss_in", _P), ("pxpy", _P)]


@functools.lru_cache(maxsize=None)
def pbr_soft_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    L.rps_render.restype = ctypes.c_int
    L.rps_render.argtypes = [ctypes.POINTER(R.RefFrame), ctypes.POINTER(P.RefConsts), ctypes.POINTER(S.RefPcss), ctypes.POINTER(P.RefIbl),
                             ctypes.POINTER(R.RefDraw), ctypes.POINTER(P.RefMaterial), ctypes.c_int, ctypes.POINTER(R.RefPlanes),
                             ctypes.POINTER(P.RefDebugPlanes), ctypes.POINTER(RefPcssPlanes)]
    L.rps_fragments.restype = ctypes.c_int
    L.rps_fragments.argtypes = [ctypes.POINTER(R.RefFrame), ctypes.POINTER(P.RefConsts), ctypes.POINTER(S.RefPcss), ctypes.POINTER(P.RefIbl),
                                ctypes.c_int, _P, _P, _P, ctypes.POINTER(P.RefMaterial)] + [_P] * 7
    return L


def pbr_soft_frame(view, light_vp, w=W, h=H, tile=(80, 80), **kw):
    return R._frame(view, light_vp, w, h, tile, shading=3, **kw)


def ref_render_pbr_soft(frame, draws, mats, shadow=None, ibl=None, consts=None, pcss=None):
    """PASS1 of hello_pbr_light_shafts.cpp for a shs_gpu.RtFrame -> test_canvas_rt_pbr_ref.ref_render_pbr's planes and
    counters, plus 'blockers', 'radius', 'pcss_flags', 'pcss_in' [.., 4] (uv.x, uv.y, z, bias) and 'pxpy' [.., 2]."""
    Wd, Hd = frame.width, frame.height
    keep = []
    arr = R._ref_draws(draws, keep)
    f = P._frame_c(frame, shadow, keep)
    out = {"color": np.empty((Hd, Wd, 4), np.uint8), "depth": np.empty((Hd, Wd), F), "velocity": np.empty((Hd, Wd, 2), F),
           "prequant": np.empty((Hd, Wd, 4), F), "tri_id": np.empty((Hd, Wd), np.int32), "texel": np.empty((Hd, Wd), np.int32),
           "flags": np.empty((Hd, Wd), np.int32)}
    dbg = {k: np.empty((Hd, Wd), np.int32) for k in ("face_n", "face_r", "m0", "m1", "pbr_flags")}
    dbg.update(prepow=np.empty((Hd, Wd, 3), F), frag_in=np.empty((Hd, Wd, 6), F), base=np.empty((Hd, Wd, 3), np.uint8))
    sdbg = {"blockers": np.empty((Hd, Wd), np.int32), "radius": np.empty((Hd, Wd), F), "pcss_flags": np.empty((Hd, Wd), np.int32),
            "pcss_in": np.empty((Hd, Wd, 4), F), "pxpy": np.empty((Hd, Wd, 2), np.int32)}
    p, g, sg = R.RefPlanes(), P.RefDebugPlanes(), RefPcssPlanes()
    for planes, c in ((out, p), (dbg, g), (sdbg, sg)):
        for k, v in planes.items():
            setattr(c, k, v.ctypes.data)
    kc, ic, pc = P._consts_c(consts), P._ibl_c(ibl, keep), S._pcss_c(pcss)
    assert pbr_soft_lib().rps_render(ctypes.byref(f), ctypes.byref(kc), ctypes.byref(pc), None if ic is None else ctypes.byref(ic), arr,
                                     P._materials_c(mats), len(draws), ctypes.byref(p), ctypes.byref(g), ctypes.byref(sg)) == 0
    out.update(dbg)
    out.update(sdbg)
    out["counters"] = dict(zip(("input_tris", "polys3", "polys4", "sub_tris"), (int(c) for c in p.counters)))
    return out


def ref_fragments_soft(frame, normal, world, base, mats, pxpy, shadow=None, ibl=None, consts=None, pcss=None):
    """fragment_shader_pbr :768-850 of n fragments -> (pre [n, 4], prepow [n, 3], rgba [n, 4], debug [n, 5],
    pcss debug [n, 3]: blockers, flags, the radius' bits, pcss_in [n, 4])"""
    keep = []
    f = P._frame_c(frame, shadow, keep)
    normal, world = np.ascontiguousarray(normal, F).reshape(-1, 3), np.ascontiguousarray(world, F).reshape(-1, 3)
    n = normal.shape[0]
    base = np.ascontiguousarray(base, np.uint8).reshape(n, 3)
    pxpy = np.ascontiguousarray(pxpy, np.int32).reshape(n, 2)
    pre, prepow, rgba, dbg = np.empty((n, 4), F), np.empty((n, 3), F), np.empty((n, 4), np.uint8), np.empty((n, 5), np.int32)
    sdbg, pin = np.empty((n, 3), np.int32), np.empty((n, 4), F)
    kc, ic, pc = P._consts_c(consts), P._ibl_c(ibl, keep), S._pcss_c(pcss)
    assert pbr_soft_lib().rps_fragments(ctypes.byref(f), ctypes.byref(kc), ctypes.byref(pc), None if ic is None else ctypes.byref(ic), n,
                                        normal.ctypes.data, world.ctypes.data, base.ctypes.data, P._materials_c(mats), pxpy.ctypes.data,
                                        pre.ctypes.data, prepow.ctypes.data, rgba.ctypes.data, dbg.ctypes.data, sdbg.ctypes.data,
                                        pin.ctypes.data) == 0
    return pre, prepow, rgba, dbg, sdbg, pin


# ---- what fails without the feature, without a GPU ---------------------------------------------------------

def test_library_exports_the_entry_point_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in ("shs_rt_render_pbr_soft", "shs_rt_render_pbr", "shs_rt_render", "shs_rt_set_pcss", "shs_rt_set_pbr"):
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1
    with open(os.path.join(ROOT, "include", "shs_gpu.h")) as fh:
        header = fh.read()
    assert "int shs_rt_render_pbr_soft(shs_ctx *ctx, const shs_rt_frame *frame, const shs_rt_draw *draws" in header


def test_structs_keep_their_sizes(tmp_path):
    """No struct changed size for the new entry point: the header's sizes are the ctypes mirrors', as before."""
    from shs_gpu import _abi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(shs_rt_pbr_draw), '
                   'sizeof(shs_rt_pbr), sizeof(shs_rt_frame), sizeof(shs_rt_draw), sizeof(shs_rt_pcss)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_abi.RtPbrDrawC), ctypes.sizeof(_abi.RtPbrC), ctypes.sizeof(_abi.RtFrameC), ctypes.sizeof(_abi.RtDrawC),
                     ctypes.sizeof(_abi.RtPcssC)]
    assert sizes[:2] == [60, 12] and sizes[4] == 28


# ---- cross-pin 1: shading 2's restatement ------------------------------------------------------------------

def _without_ao(mats):
    import dataclasses
    return [dataclasses.replace(m, ao=0.0) for m in mats]


@pytest.mark.parametrize("name", ("demo",) + EDGE_NAMES)
def test_without_a_map_and_ao_it_is_shading_2s_frame(name):
    """No map: both shadow factors are 1.  ao = 0: the IBL term is multiplied by 0 in both, and shading 2's minimum
    ambient base * 0.03 * 0 adds +0 to a sum that is never -0 (direct >= 0, plus ibl * 0).  Everything else is one text."""
    scenes = [P.demo_scene()] if name == "demo" else [P.edge_scene(name, which) for which in ("rough", "metal")]
    for view, lvp, draws, mats in scenes:
        mats = _without_ao(mats)
        ibl = P.make_ibl()
        soft = ref_render_pbr_soft(pbr_soft_frame(view, lvp, use_shadow=False), draws, mats, None, ibl)
        pbr = P.ref_render_pbr(P.pbr_frame(view, lvp, use_shadow=False), draws, mats, None, ibl)
        for k in ("color", "depth", "velocity", "prequant", "tri_id", "texel", "prepow", "frag_in", "base", "face_n", "face_r", "m0", "m1",
                  "pbr_flags"):
            assert np.array_equal(soft[k].view(np.uint8), pbr[k].view(np.uint8)), (name, k)
        assert soft["counters"] == pbr["counters"]
        shaded = soft["tri_id"] >= 0
        assert shaded.sum() > 1000 and (soft["pcss_flags"][shaded] == NOT_IN_LIGHT).all()
        assert name != "demo" or (soft["prequant"][..., :3][shaded] > 0).sum() > 10000


# ---- cross-pin 2: the soft demo's PCSS text ----------------------------------------------------------------

GPU_PCSS = {"demo": None, "wide": S.WIDE, "no-blockers": dict(blocker_samples=0), "no-taps": dict(pcf_samples=0),
            "wrap": dict(pcf_samples=40), "wide-light": dict(light_uv_radius=0.05)}


@functools.lru_cache(maxsize=None)
def demo_planes(pcss="demo", sm=SM, tile=80, casters_from=0, size=(W, H)):
    """(shadow map, shading 3's planes) of the demo in miniature under make_ibl(); casters_from = 1 leaves the floor out
    of PASS0, so its fragments find empty centre texels."""
    view, lvp, draws, mats = P.demo_scene()
    if size != (W, H):
        view, proj = R.camera(*size)
        draws = [R._rt_draw(d.mesh, d.model, view, proj, color=d.base_color, tex=d.albedo_tex) for d in draws]
    shadow = R.ref_shadow(sm, lvp, draws[casters_from:], (tile, tile))
    k = None if GPU_PCSS[pcss] is None else S.demo_pcss(**GPU_PCSS[pcss])
    return shadow, ref_render_pbr_soft(pbr_soft_frame(view, lvp, size[0], size[1], (tile, tile)), draws, mats, shadow, P.make_ibl(), pcss=k)


@functools.lru_cache(maxsize=None)
def edge_planes(name, which, pcss="demo"):
    view, lvp, draws, mats = P.edge_scene(name, which)
    shadow = R.ref_shadow(SM, lvp, draws)
    k = None if GPU_PCSS[pcss] is None else S.demo_pcss(**GPU_PCSS[pcss])
    return shadow, ref_render_pbr_soft(pbr_soft_frame(view, lvp), draws, mats, shadow, P.make_ibl(), pcss=k)


def _assert_factor_plane_is_the_soft_texts(shadow, out, pcss):
    called = (out["tri_id"] >= 0) & ((out["pcss_flags"] & NOT_IN_LIGHT) == 0)
    pin, pxpy = out["pcss_in"][called], out["pxpy"][called]
    fac, blockers, radius, flags = S.ref_pcss_samples(shadow, pin[:, :2], pin[:, 2], pin[:, 3], pxpy, pcss)
    assert np.array_equal(fac.view(np.uint32), out["prequant"][..., 3][called].view(np.uint32))
    assert np.array_equal(blockers, out["blockers"][called]) and np.array_equal(radius.view(np.uint32), out["radius"][called].view(np.uint32))
    assert np.array_equal(flags, out["pcss_flags"][called] & 127)
    rest = (out["tri_id"] >= 0) & ~called
    assert (out["prequant"][..., 3][rest] == 1.0).all()
    # the screen pixel handed to the shader is the pixel itself, screen rows
    ys, xs = np.nonzero(out["tri_id"] >= 0)
    hh = out["tri_id"].shape[0]
    assert np.array_equal(out["pxpy"][ys, xs], np.stack([xs, hh - 1 - ys], -1))
    return int(called.sum())


def test_factor_plane_is_the_soft_demos_pcss_of_the_reported_inputs():
    """The legacy ShadowMap returns FLT_MAX out of bounds where the soft demo's clamps; shadow_sample_depth_uv looks at
    neither outside [0, 1], so both texts agree on every shaded pixel, taps off the map included."""
    n = 0
    for key, kw in (("demo", {}), ("wide", {}), ("wrap", {}), ("demo", dict(casters_from=1)), ("wide", dict(sm=(96, 40))), ("demo", dict(sm=(1, 1)))):
        shadow, out = demo_planes(key, **kw)
        n += _assert_factor_plane_is_the_soft_texts(shadow, out, None if GPU_PCSS[key] is None else S.demo_pcss(**GPU_PCSS[key]))
    for name in EDGE_NAMES:
        shadow, out = edge_planes(name, "rough")
        n += _assert_factor_plane_is_the_soft_texts(shadow, out, None)
    assert n > 50000


# ---- known answers for the three differences ---------------------------------------------------------------

def _one(frame, n, wp, base, mat, pxpy=(3, 4), **kw):
    pre, prepow, rgba, dbg, sdbg, pin = ref_fragments_soft(frame, [n], [wp], [base], [mat], [pxpy], **kw)
    return pre[0], prepow[0], rgba[0], sdbg[0]


def test_known_answers_for_the_three_differences():
    view, lvp, _, _ = P.demo_scene()
    eye = np.eye(4, dtype=F).reshape(16)
    lit, p5, base = (0.2, 0.9, -0.4), (0.1, 0.2, 0.5), (200, 120, 40)
    m = P.material(metallic=0.3, roughness=0.5, ao=0.6)
    # (1) no ambient: a fully blocked pixel over a flat map (identity light_vp, z = 0.5 behind a 256^2 map of zeros,
    # whose 28-texel filter stays on the map) without an
    # IBL encodes to exactly 0, bytes and floats, where shading 2 gives the minimum ambient
    fs = pbr_soft_frame(view, eye, use_shadow=True)
    pre, prepow, rgba, sdbg = _one(fs, lit, p5, base, m, shadow=np.zeros((256, 256), F))
    assert pre[3] == 0.0 and sdbg[0] == 12 and not (pre[:3] != 0).any() and not (prepow != 0).any() and tuple(rgba) == (0, 0, 0, 255)
    p2 = P.ref_fragments(P.pbr_frame(view, eye, use_shadow=True), [lit], [p5], [base], [m], np.zeros((256, 256), F))[0][0]
    assert p2[3] == 0.0 and (p2[:3] > 0).all()
    assert _one(fs, lit, p5, base, m, shadow=np.ones((256, 256), F))[0][3] == 1.0
    # (2) SHS_RT_PCF set or clear: the same frame
    _, lvp2, draws, mats = P.demo_scene()
    shadow = R.ref_shadow(SM, lvp2, draws)
    a = ref_render_pbr_soft(pbr_soft_frame(view, lvp2, pcf=True), draws, mats, shadow, P.make_ibl())
    b = ref_render_pbr_soft(pbr_soft_frame(view, lvp2, pcf=False), draws, mats, shadow, P.make_ibl())
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("color", "prequant", "depth", "velocity", "pcss_in"))
    assert ((a["prequant"][..., 3] > 0) & (a["prequant"][..., 3] < 1)).sum() > 1000
    # (3) direct_intensity scales the direct term only: at intensity 0 a lit fragment is the IBL term alone, which is the
    # fully shadowed fragment's colour at any intensity; without an IBL it is 0; and twice the intensity doubles the
    # linear colour of an IBL-less fragment exactly (x -> x / (1 + x) undone in float64)
    ibl = P.make_ibl()
    f0 = pbr_soft_frame(view, lvp, use_shadow=False)
    dark = _one(f0, lit, p5, base, m, ibl=ibl, consts=P.demo_consts(direct_intensity=0.0))
    blocked = _one(fs, lit, p5, base, m, shadow=np.zeros((256, 256), F), ibl=ibl, consts=P.demo_consts(direct_intensity=7.0))
    assert np.array_equal(dark[1], blocked[1]) and (dark[1] > 0).all()
    assert not _one(f0, lit, p5, base, m, consts=P.demo_consts(direct_intensity=0.0))[1].any()
    one = _one(f0, lit, p5, base, m, consts=P.demo_consts(direct_intensity=1.5))[1].astype(np.float64)
    two = _one(f0, lit, p5, base, m, consts=P.demo_consts(direct_intensity=3.0))[1].astype(np.float64)
    lin1, lin2 = one / (1 - one), two / (1 - two)
    assert (one > 0).all() and np.allclose(lin2, 2 * lin1, rtol=1e-5)
    with_ibl = _one(f0, lit, p5, base, m, ibl=ibl)[1].astype(np.float64)
    d = dark[1].astype(np.float64)
    assert np.allclose(with_ibl / (1 - with_ibl) - d / (1 - d), lin2, rtol=1e-4)      # the default intensity is the demo's 3.0


# ---- the second restatement: float32 numpy -----------------------------------------------------------------

def _m4v(m16, p):
    """glm's mat4 * vec4(p, 1), column-major: (m0 x + m1 y) + (m2 z + m3 w), as the C files' mat4_vec4"""
    m = np.asarray(m16, F).reshape(4, 4)   # m[c][r]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return [(m[0, r] * x + m[1, r] * y) + (m[2, r] * z + m[3, r] * F(1)) for r in range(4)]


def np_shadow_inputs(frame, N, world):
    """shadow_uvz_from_world :558-576 and the bias of :814-815 -> (called [n], uv [n, 2], z [n], bias [n])"""
    cx, cy, cz, cw = _m4v(frame.light_vp, np.asarray(world, F))
    with np.errstate(all="ignore"):
        nx, ny, z = cx / cw, cy / cw, cz / cw
        called = ~(np.abs(cw) < F(1e-6)) & ~((z < 0) | (z > 1))
        uv = np.stack([nx * F(0.5) + F(0.5), F(1) - (ny * F(0.5) + F(0.5))], -1).astype(F)
    L = P._normalize(-np.asarray(frame.light_dir_world, F))[None, :]
    ndl = P._dot(N, np.broadcast_to(L, N.shape))
    slope = F(1) - np.minimum(np.maximum(ndl, F(0)), F(1))
    bias = (F(frame.bias_base) + F(frame.bias_slope) * slope).astype(F)
    return called, uv, z.astype(F), bias


def np_fragments_soft(frame, normal, world, base, mats, pxpy, shadow_map, ibl, consts, pcss):
    """fragment_shader_pbr (hello_pbr_light_shafts.cpp:768-850) in float32 numpy over n fragments, the PCSS factor from
    test_canvas_rt_soft_ref.np_pcss.  mats: a dict of [n] arrays.  -> (prepow [n, 3], pre [n, 3], factor [n])"""
    k = P.demo_consts() if consts is None else consts
    N = P._normalize(np.asarray(normal, F))
    V = P._normalize(np.asarray(frame.camera_pos, F)[None, :] - np.asarray(world, F))
    L = P._normalize(-np.asarray(frame.light_dir_world, F))[None, :]
    Hh = P._normalize(V + L)
    zero = F(0)
    mx0 = lambda x: np.where(zero < x, x, zero).astype(F)   # noqa: E731  glm::max(0, x)
    NoV, NoL, NoH = mx0(P._dot(N, V)), mx0(P._dot(N, np.broadcast_to(L, N.shape))), mx0(P._dot(N, Hh))
    lin = P._powf_table()[np.asarray(base, np.uint8)]
    metallic = P._sat(mats["metallic"])
    r = mats["roughness"].astype(F)
    roughness = np.where(r < F(k.min_roughness), F(k.min_roughness), np.where(r > F(1), F(1), r)).astype(F)
    ao = P._sat(mats["ao"])
    om = F(1) - metallic
    F0 = F(0.04) * om[:, None] + lin * metallic[:, None]
    x = F(1) - P._sat(NoV)
    x2 = x * x
    x5 = (x2 * x2 * x)[:, None]
    Fr = (F0 + (F(1) - F0) * x5) * np.array([1.0, 0.96, 0.90], F)[None, :]
    kd = (F(1) - Fr) * om[:, None]
    PI = F(3.14159265358979323846)
    a2 = (roughness * roughness) * (roughness * roughness)
    nh = P._sat(NoH)
    dd = (nh * nh) * (a2 - F(1)) + F(1)
    D = a2 / (PI * dd * dd)
    r1 = roughness + F(1)
    kk = (r1 * r1) / F(8)
    gs = lambda c: P._sat(c) / (P._sat(c) * (F(1) - kk) + kk)   # noqa: E731
    G = gs(NoV) * gs(NoL)
    den = np.where(F(1e-6) < F(4) * NoV * NoL, F(4) * NoV * NoL, F(1e-6)).astype(F)
    direct = (kd * lin * (F(1) / PI) + ((D * G)[:, None] * Fr) / den[:, None]) * F(k.direct_intensity) * NoL[:, None]
    factor = np.ones(len(N), F)
    if frame.use_shadow:
        called, uv, z, bias = np_shadow_inputs(frame, N, world)
        pk = S.demo_pcss() if pcss is None else pcss
        factor[called] = S.np_pcss(shadow_map, uv[called], z[called], bias[called], np.asarray(pxpy)[called], pk)[0]
    direct = direct * factor[:, None]
    amb = np.zeros_like(direct)
    if ibl is not None:
        irr, spec = ibl
        diff = P.np_cube(irr, N)[0] * lin * kd * P._sat(mats["ibl_diffuse_intensity"])[:, None]
        I = -V
        R_ = I - N * P._dot(N, I)[:, None] * F(2)
        pre = P.np_trilinear(spec, R_, roughness * F(len(spec) - 1))[0]
        ss = P._sat(mats["ibl_specular_intensity"]) * P._sat(mats["ibl_reflection_strength"])
        amb = diff + pre * Fr * ss[:, None]
    c = direct + amb * ao[:, None]
    c = c * F(k.exposure)
    c = c / (F(1) + c)
    prepow = np.minimum(np.maximum(c, F(0)), F(1)).astype(F)
    srgb = np.power(prepow, F(1.0) / F(2.2)).astype(F)
    return prepow, (np.minimum(np.maximum(srgb, F(0)), F(1)) * F(255)).astype(F), factor


def _assert_second_restatement(frame, normal, world, base, mats_arr, pxpy, ref_pre, ref_prepow, ref_rgba, shadow, ibl, consts, pcss):
    np_prepow, np_pre, factor = np_fragments_soft(frame, normal, world, base, mats_arr, pxpy, shadow, ibl, consts, pcss)
    assert np.array_equal(factor.view(np.uint32), np.ascontiguousarray(ref_pre[:, 3]).view(np.uint32)), "the PCSS factor"
    bad = np.argwhere(np_prepow.view(np.uint32) != np.ascontiguousarray(ref_prepow).view(np.uint32))
    assert bad.size == 0, f"{len(bad)} of {ref_prepow.size} channels differ before the pow, first {bad[:4].tolist()}"
    np_rgba = np.concatenate([np_pre.astype(np.uint8), np.full((len(np_pre), 1), 255, np.uint8)], axis=1)
    helpers.assert_color_parity(np_rgba[None], ref_rgba[None], np_pre[None], ref_pre[None, :, :3])


def test_numpy_restatement_on_random_fragments():
    view, lvp, draws, _ = P.demo_scene()
    shadow = R.ref_shadow(SM, lvp, draws)
    normal, world, base, mats = P.random_fragments(seed=33, n=1500)
    pxpy = np.random.default_rng(34).integers(0, 800, (len(normal), 2)).astype(np.int32)
    for ibl, consts, pcss, use_shadow in ((P.make_ibl(), None, None, True), (None, None, None, False),
                                          (P.make_ibl(3, 5, 6, 3), P.demo_consts(exposure=0.9, min_roughness=0.1, direct_intensity=5.0),
                                           S.demo_pcss(**S.WIDE), True)):
        frame = pbr_soft_frame(view, lvp, use_shadow=use_shadow)
        sm = shadow if use_shadow else None
        pre, prepow, rgba, _, sdbg, _ = ref_fragments_soft(frame, normal, world, base, mats, pxpy, sm, ibl, consts, pcss)
        _assert_second_restatement(frame, normal, world, base, P._mats_arrays(mats), pxpy, pre, prepow, rgba, sm, ibl, consts, pcss)
        if use_shadow:
            assert ((pre[:, 3] > 0) & (pre[:, 3] < 1)).sum() > 30 and (pre[:, 3] == 0).sum() > 30


def test_numpy_restatement_on_every_pixel_of_a_small_frame():
    shadow, ref = demo_planes(sm=50, size=(40, 30))
    view, lvp, draws, mats = P.demo_scene()
    frame = pbr_soft_frame(view, lvp, 40, 30)
    px = ref["tri_id"] >= 0
    assert px.sum() > 500
    who = np.searchsorted(np.cumsum([d.mesh.positions.shape[0] for d in draws]), ref["tri_id"][px] // 2, side="right")
    assert set(who.tolist()) == {0, 1, 2}
    fi = ref["frag_in"][px]
    _assert_second_restatement(frame, fi[:, :3], fi[:, 3:], ref["base"][px], P._mats_arrays(mats, who), ref["pxpy"][px], ref["prequant"][px],
                               ref["prepow"][px], ref["color"][px], shadow, P.make_ibl(), None, None)
    # numpy's shadow_uvz_from_world and bias are the C file's bits
    called, uv, z, bias = np_shadow_inputs(frame, P._normalize(fi[:, :3]), fi[:, 3:])
    assert np.array_equal(called, (ref["pcss_flags"][px] & NOT_IN_LIGHT) == 0) and called.sum() > 400
    want = ref["pcss_in"][px][called]
    assert np.array_equal(np.concatenate([uv, z[:, None], bias[:, None]], 1)[called].view(np.uint32), want.view(np.uint32))


# ---- what the GPU frames are there for ---------------------------------------------------------------------

def seen(out, hi):
    shaded = out["tri_id"] >= 0
    fl, fac = out["pcss_flags"], out["prequant"][..., 3]
    cnt = lambda bit: int((shaded & ((fl & bit) != 0)).sum())   # noqa: E731
    return {"uv_outside": cnt(UV_OUTSIDE), "empty_centre": cnt(EMPTY_CENTRE), "no_blocker": cnt(NO_BLOCKER),
            "partial": int((shaded & (fac > 0) & (fac < 1)).sum()), "dark": int((shaded & (fac == 0)).sum()),
            "radius_min": cnt(RADIUS_AT_MIN), "radius_max": cnt(RADIUS_AT_MAX),
            "radius_between": int((shaded & (out["radius"] >= 0) & ((fl & (RADIUS_AT_MIN | RADIUS_AT_MAX)) == 0)).sum()),
            "tap_off_map": cnt(BLOCKER_OFF_MAP | PCF_OFF_MAP), "pcf_off_map": cnt(PCF_OFF_MAP), "tap_empty": cnt(BLOCKER_EMPTY | PCF_EMPTY),
            "not_in_light": cnt(NOT_IN_LIGHT), "textured": int((out["texel"] >= 0).sum()), "moving": int(out["velocity"].any(-1).sum())}


# Minimum pixel counts per frame of tests/test_canvas_rt_pbr_soft.py, counted from this restatement alone; beside each,
# in the comment, what it shows (x86-64, glibc).  Every class the shader's PCSS can reach is met by one of them.
NEED = {
    # the miniature over 96^2 under the demo's constants: 0.0035 * ratio * 96 < 1, every radius at the minimum; the
    # 18-texel search leaves the map at its border.   partial 7650, dark 153, radius_min 12723 (no other radius),
    # no_blocker 742, tap_off_map 2865, uv_outside 617, textured 942, moving 657
    "demo": dict(partial=3000, dark=40, radius_min=6000, no_blocker=300, tap_off_map=1400, uv_outside=300, textured=300, moving=300),
    # the widened constants: radii between the clamps and at the maximum, PCF taps off the map.
    # partial 12158, radius_min 525, radius_between 10464, radius_max 1734, pcf_off_map 43
    "demo-wide": dict(partial=6000, radius_min=250, radius_between=5000, radius_max=800, pcf_off_map=20),
    # the floor left out of PASS0: empty centre texels, taps on empty texels.   empty_centre 11770, tap_empty 1695
    "demo-objects": dict(empty_centre=5000, tap_empty=800),
    # the small light box of the 'outside' scene: receivers outside its depth range and extent.
    # not_in_light 6004, uv_outside 6572
    "outside": dict(not_in_light=3000, uv_outside=3000),
    # a 96 x 40 map under the widened constants.   partial 12763, radius_max 3279, tap_off_map 9866
    "demo-wide-96x40": dict(partial=6000, radius_max=1500, tap_off_map=3500),
}


def test_frames_cover_what_the_gpu_tests_need():
    frames = {"demo": (demo_planes()[1], 28.0), "demo-wide": (demo_planes("wide")[1], 3.0),
              "demo-objects": (demo_planes(casters_from=1)[1], 28.0), "outside": (edge_planes("outside", "rough")[1], 28.0),
              "demo-wide-96x40": (demo_planes("wide", sm=(96, 40))[1], 3.0)}
    for key, (out, hi) in frames.items():
        got = seen(out, hi)
        print(key, got)
        short = {k: (got[k], v) for k, v in NEED[key].items() if got[k] < v}
        assert not short, (key, short)
    assert seen(demo_planes()[1], 28.0)["radius_max"] == 0 and seen(demo_planes()[1], 28.0)["radius_between"] == 0


# ---- the texel a textured pixel samples, pinned by sensitivity ---------------------------------------------

# Shading 2's tests read the sampled texel back from a frame whose colour is the minimum ambient alone, a function of the
# base colour and nothing else.  This shader has no such term.  Under direct_intensity = 0, an all-ones irradiance and
# ibl_specular_intensity = 0 its colour is encode(base * kd(NoV) * ao * exposure): the texel's bytes times a factor that
# varies slowly over the quad.  TEX codes texel (x, y) as r = 10 + 5 x, g = 10 + 7 y; under an exposure of 30 the linear
# values 0.0008 .. 0.09 land on the steep part of x / (1 + x), and a neighbouring texel moves a channel by far more than
# the GPU test's bar on the floats.
TEXEL_CONSTS = dict(exposure=30.0, direct_intensity=0.0)


def ones_ibl():
    irr, spec = P.make_ibl()
    return np.ones_like(irr), spec


@functools.lru_cache(maxsize=None)
def texel_frame():
    """(frame, draws, mats, ibl, consts, the restatement's planes) of the texel-identity frame."""
    import dataclasses
    view, lvp, draws, mats = P.demo_scene()
    mats = [dataclasses.replace(m, ibl_specular_intensity=0.0) for m in mats]
    frame = pbr_soft_frame(view, lvp, use_shadow=False)
    consts = P.demo_consts(**TEXEL_CONSTS)
    return frame, draws, mats, ones_ibl(), consts, ref_render_pbr_soft(frame, draws, mats, None, ones_ibl(), consts)


def texel_sensitivity():
    """Per textured pixel of texel_frame(): the smallest, over the texel's neighbours in the texture, of the largest
    channel difference (pre-truncation floats) the neighbour's bytes would make."""
    frame, draws, mats, ibl, consts, ref = texel_frame()
    px = ref["texel"] >= 0
    who = np.searchsorted(np.cumsum([d.mesh.positions.shape[0] for d in draws]), ref["tri_id"][px] // 2, side="right")
    assert len(set(who.tolist())) == 1
    d, mat = draws[int(who[0])], mats[int(who[0])]
    rgba = np.asarray(d.albedo_tex.rgba, np.uint8)
    th, tw = rgba.shape[:2]
    fi, idx, own = ref["frag_in"][px], ref["texel"][px], ref["prequant"][px][:, :3]
    ty, tx = idx // tw, idx % tw
    assert np.array_equal(rgba[ty, tx][:, :3], ref["base"][px])
    least = np.full(len(idx), np.inf)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ny, nx = ty + dy, tx + dx
            ok = ((dy, dx) != (0, 0)) & (ny >= 0) & (ny < th) & (nx >= 0) & (nx < tw)
            if not np.any(ok):
                continue
            pre = ref_fragments_soft(frame, fi[ok][:, :3], fi[ok][:, 3:], rgba[ny[ok], nx[ok]][:, :3], [mat] * int(ok.sum()),
                                     ref["pxpy"][px][ok], None, ibl, consts)[0]
            least[ok] = np.minimum(least[ok], np.abs(pre[:, :3].astype(np.float64) - own[ok]).max(1))
    return least


def test_a_neighbouring_texel_would_move_the_texel_frame():
    least = texel_sensitivity()
    share = float((least > 10 * helpers.TOL * 255.0).mean())
    print(f"{len(least)} textured pixels, {100 * share:.2f} % would move by more than 10x the bar under any neighbouring texel "
          f"(smallest move {least.min():.3g})")
    assert len(least) > 300 and share >= 0.95


# ---- the demo's whole frame --------------------------------------------------------------------------------

SHAFT_PARAMS = dict(steps=8)


def chain_sky():
    import test_canvas_rt_sky_ref as K
    return dict(K.demo_skies())["analytic"]


def shafts_inputs(color, depth, shadow, light_vp):
    """test_canvas_light_shafts_ref's input dict over a rendered frame's planes and PASS0's map."""
    import test_canvas_light_shafts_ref as L
    h, w = depth.shape
    view, proj = R.camera(w, h)
    return dict(w=w, h=h, cam_pos=R.CAM_POS, inv_vp=L.inverse16(R._mul(proj, view)), light_vp=np.asarray(light_vp, F).reshape(16),
                sun=L.SUN_DIR, shadow=np.ascontiguousarray(shadow, F), depth=np.ascontiguousarray(depth, F),
                src=np.ascontiguousarray(color, np.uint8))


def test_the_restatement_chain_marches_enough_pixels_for_the_cap_to_bind():
    """PASS0 -> sky -> shading 3 -> light shafts at 160 x 120 with 8 steps, the restatements alone: the GPU test's cap of
    1 differing step count in 2,000 marched pixels allows at least one pixel only above 2,000."""
    import test_canvas_light_shafts_ref as L
    import test_canvas_rt_sky_ref as K
    view, lvp, draws, mats = P.demo_scene()
    shadow = R.ref_shadow(SM, lvp, draws, (160, 160))
    plain = ref_render_pbr_soft(pbr_soft_frame(view, lvp, tile=(160, 160)), draws, mats, shadow, P.make_ibl())
    ref = K.ref_compose(chain_sky(), plain)
    out = L.ref_pass(shafts_inputs(ref["color"], ref["depth"], shadow, lvp), SHAFT_PARAMS)
    n = int(L.marched(out["pq"]).sum())
    print(f"{n} marched pixels, cap {L.step_cap(n)}")
    assert n > 2000 and L.step_cap(n) >= 1 and (out["color"] != ref["color"]).any()
