"""tests/canvas_rt_soft_ref (ref_canvas_rt_soft.c), the C restatement of hello_shadow_mapping_soft.cpp's camera
pass and PCSS shadow factor -- the reference of tests/test_canvas_rt_soft.py -- pinned on the CPU:

  * hash_u32 / hash01 and the pixel seed against Python integers;
  * pcss_shadow_factor against a second restatement in float32 numpy, written from the same cited lines, whose
    cos / sin are libm's cosf / sinf through ctypes (numpy's float32 cos is another implementation);
  * by known answers at every early-out and edge of pcss_shadow_factor (known_cases, shared with the GPU test);
  * without a shadow map its raster is test_canvas_rt_ref's (the same depth, sub-triangles and counters);
  * and the scenes of the GPU tests are checked to show, in the restatement's debug planes, what they are there for.

It also holds what fails without the feature and needs no GPU: the new entry points and shs_rt_pcss's size."""
import ctypes
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers
import test_canvas_rt_ref as R
from test_canvas_rt_ref import F, FLT_MAX, H, SM, W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_soft_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_soft_ref.so")
_P = ctypes.c_void_p
UV_OUTSIDE, EMPTY_CENTRE, NO_BLOCKER, BLOCKER_OFF_MAP, BLOCKER_EMPTY, PCF_OFF_MAP, PCF_EMPTY, NOT_IN_LIGHT = 1, 2, 4, 8, 16, 32, 64, 128
TWO_PI = F(6.2831853)


class RefPcss(ctypes.Structure):
    _fields_ = [("light_uv_radius", ctypes.c_float), ("search_radius_texels", ctypes.c_float), ("min_filter_texels", ctypes.c_float),
                ("max_filter_texels", ctypes.c_float), ("epsilon", ctypes.c_float), ("blocker_samples", ctypes.c_int32),
                ("pcf_samples", ctypes.c_int32)]


class RefDebugPlanes(ctypes.Structure):
    _fields_ = [("blockers", _P), ("radius", _P), ("pcss_flags", _P)]


def demo_pcss(**kw):
    """shs_gpu.RtPcss with the demo's constants (hello_shadow_mapping_soft.cpp:101-116), some replaced."""
    import shs_gpu
    return dataclasses.replace(shs_gpu.RtPcss(), **kw)


# The widened set.  On a 96-texel map the demo's 0.0035 keeps every radius at the min clamp: the radius in texels is
# light * ratio * 96 and the miniature's penumbra ratios (zR - zB) / zB lie below 0.35 (its light spans 40 units of
# depth), so a light of 0.05 with a max of 6 texels still leaves all but a few at the min clamp.  0.3 with a max of
# 3 texels puts ratio 0.035 at the min clamp and 0.104 at the max: the radii span both.
WIDE = dict(light_uv_radius=0.3, max_filter_texels=3.0)


def _pcss_c(p):
    p = demo_pcss() if p is None else p
    return RefPcss(p.light_uv_radius, p.search_radius_texels, p.min_filter_texels, p.max_filter_texels, p.epsilon,
                   int(p.blocker_samples), int(p.pcf_samples))


@functools.lru_cache(maxsize=None)
def soft_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    L.rcs_render.restype = ctypes.c_int
    L.rcs_render.argtypes = [ctypes.POINTER(R.RefFrame), ctypes.POINTER(RefPcss), ctypes.POINTER(R.RefDraw), ctypes.c_int,
                             ctypes.POINTER(R.RefPlanes), ctypes.POINTER(RefDebugPlanes)]
    L.rcs_pcss_samples.restype = ctypes.c_int
    L.rcs_pcss_samples.argtypes = [_P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RefPcss), ctypes.c_int] + [_P] * 8
    L.rcs_hash_u32.restype = ctypes.c_uint32
    L.rcs_hash_u32.argtypes = [ctypes.c_uint32]
    L.rcs_hash01.restype = ctypes.c_float
    L.rcs_hash01.argtypes = [ctypes.c_uint32]
    L.rcs_pixel_seed.restype = ctypes.c_uint32
    L.rcs_pixel_seed.argtypes = [ctypes.c_int, ctypes.c_int]
    L.rcs_rotation.restype = None
    L.rcs_rotation.argtypes = [ctypes.c_int, ctypes.c_int, _P, _P]
    L.rcs_rotated_tap.restype = None
    L.rcs_rotated_tap.argtypes = [ctypes.c_int] * 4 + [_P]
    return L


def ref_render_soft(frame, draws, shadow=None, pcss=None):
    """The soft PASS1 of a shs_gpu.RtFrame -> test_canvas_rt_ref.ref_render's planes and counters, plus the debug
    planes 'blockers', 'radius' and 'pcss_flags' (canvas rows)."""
    Wd, Hd = frame.width, frame.height
    keep = []
    arr = R._ref_draws(draws, keep)
    f = R.RefFrame()
    f.W, f.H = Wd, Hd
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
    out = {"color": np.empty((Hd, Wd, 4), np.uint8), "depth": np.empty((Hd, Wd), F), "velocity": np.empty((Hd, Wd, 2), F),
           "prequant": np.empty((Hd, Wd, 4), F), "tri_id": np.empty((Hd, Wd), np.int32), "texel": np.empty((Hd, Wd), np.int32),
           "flags": np.empty((Hd, Wd), np.int32)}
    dbg = {"blockers": np.empty((Hd, Wd), np.int32), "radius": np.empty((Hd, Wd), F), "pcss_flags": np.empty((Hd, Wd), np.int32)}
    p, g = R.RefPlanes(), RefDebugPlanes()
    for k, v in out.items():
        setattr(p, k, v.ctypes.data)
    for k, v in dbg.items():
        setattr(g, k, v.ctypes.data)
    k = _pcss_c(pcss)
    assert soft_lib().rcs_render(ctypes.byref(f), ctypes.byref(k), arr, len(draws), ctypes.byref(p), ctypes.byref(g)) == 0
    out.update(dbg)
    out["counters"] = dict(zip(("input_tris", "polys3", "polys4", "sub_tris"), (int(c) for c in p.counters)))
    return out


def ref_pcss_samples(sm, uv, z, bias, pxpy, pcss=None):
    """pcss_shadow_factor of n samples -> (factor [n], blockers [n], radius [n], flags [n])."""
    sm = np.ascontiguousarray(sm, F)
    uv = np.ascontiguousarray(uv, F).reshape(-1, 2)
    n = uv.shape[0]
    z, bias = np.ascontiguousarray(z, F).reshape(n), np.ascontiguousarray(bias, F).reshape(n)
    pxpy = np.ascontiguousarray(pxpy, np.int32).reshape(n, 2)
    out, blockers, radius, flags = np.empty(n, F), np.empty(n, np.int32), np.empty(n, F), np.empty(n, np.int32)
    k = _pcss_c(pcss)
    assert soft_lib().rcs_pcss_samples(sm.ctypes.data, sm.shape[1], sm.shape[0], ctypes.byref(k), n, uv.ctypes.data, z.ctypes.data,
                                       bias.ctypes.data, pxpy.ctypes.data, out.ctypes.data, blockers.ctypes.data,
                                       radius.ctypes.data, flags.ctypes.data) == 0
    return out, blockers, radius, flags


def soft_frame(view, light_vp, w=W, h=H, tile=(80, 80), **kw):
    return R._frame(view, light_vp, w, h, tile, shading=1, **kw)


# ---- sample sets (shared with tests/test_canvas_rt_soft.py) ----------------------------------------------------

def random_samples(seed=11, n=4096, w=64, h=40):
    """A random w x h map with about a third of its texels empty and n samples whose taps leave the map at the
    borders, with a few uv outside [0, 1] and z on both sides of the map's depths."""
    rng = np.random.default_rng(seed)
    sm = rng.uniform(0.2, 0.8, (h, w)).astype(F)
    sm[rng.random((h, w)) < 1.0 / 3.0] = FLT_MAX
    uv = rng.uniform(-0.02, 1.02, (n, 2)).astype(F)
    z = rng.uniform(0.1, 1.0, n).astype(F)
    bias = rng.uniform(0.0, 0.02, n).astype(F)
    pxpy = rng.integers(0, 2048, (n, 2)).astype(np.int32)
    return sm, uv, z, bias, pxpy


def _uniform(v, w=64, h=64):
    return np.full((h, w), v, F)


def known_cases():
    """(name, map, RtPcss or None, uv, z, bias, pxpy, expected factor, expected flag bits or None)."""
    eps1 = float(np.nextafter(F(1), F(2)))
    hole = _uniform(0.3)
    hole[31, 32] = FLT_MAX                       # texel (32, 31): u = 32 / 63, v = 31 / 63
    only0 = _uniform(FLT_MAX, 9, 7)
    only0[0, 0] = 0.1
    not0 = _uniform(0.1, 9, 7)
    not0[0, 0] = FLT_MAX
    nan = float("nan")
    return [
        ("empty-map", _uniform(FLT_MAX), None, (0.5, 0.5), 0.6, 0.0, (3, 4), 1.0, EMPTY_CENTRE),
        ("u-below", _uniform(0.2), None, (-1e-7, 0.5), 0.6, 0.0, (3, 4), 1.0, UV_OUTSIDE),
        ("u-above", _uniform(0.2), None, (eps1, 0.5), 0.6, 0.0, (3, 4), 1.0, UV_OUTSIDE),
        ("v-below", _uniform(0.2), None, (0.5, -1e-7), 0.6, 0.0, (3, 4), 1.0, UV_OUTSIDE),
        ("v-above", _uniform(0.2), None, (0.5, eps1), 0.6, 0.0, (3, 4), 1.0, UV_OUTSIDE),
        ("empty-centre", hole, None, (32.0 / 63.0, 31.0 / 63.0), 0.6, 0.0, (3, 4), 1.0, EMPTY_CENTRE),
        ("nearer", _uniform(0.2), None, (0.5, 0.5), 0.6, 0.0, (3, 4), 0.0, 0),
        ("farther", _uniform(0.9), None, (0.5, 0.5), 0.6, 0.0, (3, 4), 1.0, NO_BLOCKER),
        ("no-blocker-samples", _uniform(0.2), demo_pcss(blocker_samples=0), (0.5, 0.5), 0.6, 0.0, (3, 4), 1.0, NO_BLOCKER),
        ("no-pcf-samples", _uniform(0.2), demo_pcss(pcf_samples=0), (0.5, 0.5), 0.6, 0.0, (3, 4), 1.0, 0),
        ("corner-uv-0", _uniform(0.2), None, (0.0, 0.0), 0.6, 0.0, (7, 9), None, None),      # taps leave the map
        ("corner-uv-1", _uniform(0.2), None, (1.0, 1.0), 0.6, 0.0, (7, 9), None, None),
        ("nan-uv-texel0-blocks", only0, None, (nan, nan), 0.6, 0.0, (3, 4), 0.0, 0),         # every tap reads texel (0, 0)
        ("nan-uv-texel0-empty", not0, None, (nan, nan), 0.6, 0.0, (3, 4), 1.0, EMPTY_CENTRE),
        ("nan-u-only", only0, None, (nan, 0.0), 0.6, 0.0, (3, 4), None, None),               # column 0; taps with v < 0 are off the map
        ("one-texel-map", _uniform(0.2, 1, 1), None, (0.5, 0.5), 0.6, 0.0, (0, 0), None, None),
        ("negative-pixel", _uniform(0.2), None, (0.5, 0.5), 0.6, 0.0, (-5, -9), 0.0, 0),
    ]


def wrap_samples(seed=12, n=256):
    """A 64 x 40 map without empty texels and samples in its middle, for the count-wrap checks."""
    rng = np.random.default_rng(seed)
    sm = rng.uniform(0.2, 0.8, (40, 64)).astype(F)
    uv = rng.uniform(0.45, 0.55, (n, 2)).astype(F)
    return sm, uv, np.full(n, 0.5, F), np.zeros(n, F), rng.integers(0, 800, (n, 2)).astype(np.int32)


# ---- what fails without the feature, without a GPU ---------------------------------------------------------

def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in ("shs_rt_set_pcss", "shs_rt_pcss_samples"):
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_ctypes_pcss_struct_has_the_headers_size(tmp_path):
    import shs_gpu
    from shs_gpu import _abi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) { printf("%zu %zu\\n", sizeof(shs_rt_pcss), '
                   'sizeof(shs_rt_frame)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [ctypes.sizeof(_abi.RtPcssC), ctypes.sizeof(_abi.RtFrameC)]
    assert ctypes.sizeof(_abi.RtPcssC) == ctypes.sizeof(RefPcss) == 28
    d = shs_gpu.RtPcss()
    assert (d.light_uv_radius, d.search_radius_texels, d.min_filter_texels, d.max_filter_texels, d.epsilon, d.blocker_samples,
            d.pcf_samples) == (0.0035, 18.0, 1.0, 28.0, 1e-5, 12, 24)
    assert shs_gpu.RtFrame(1, 1, None, None, (0, 0, 1), (0, 0, 0)).shading == 0


# ---- hash and rotation ------------------------------------------------------------------------------------------

def _py_hash(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _py_seed(px, py):
    return ((px * 1973) & 0xFFFFFFFF) ^ ((py * 9277) & 0xFFFFFFFF) ^ 0x9e3779b9


def test_hash_and_seed_equal_python_integers():
    L = soft_lib()
    assert 500000 * 9277 > 2 ** 32                                   # the py product wraps 32 bits
    for px, py in [(0, 0), (1, 0), (0, 1), (799, 599), (159, 119), (3, 500000), (32766, 32766), (-5, -9)]:
        seed = _py_seed(px, py)
        assert L.rcs_pixel_seed(px, py) == seed, (px, py)
        for s in (seed, seed ^ 0xB5297A4D):
            assert L.rcs_hash_u32(s) == _py_hash(s)
            assert L.rcs_hash01(s) == (_py_hash(s) & 0xFFFFFF) / float(1 << 24)   # exact: 24 bits over 2^24
    assert _py_seed(0, 0) == 0x9e3779b9 and L.rcs_hash_u32(0) == 0
    for x in (1, 0xFFFFFFFF, 0x80000000, 12345):
        assert L.rcs_hash_u32(x) == _py_hash(x)


@functools.lru_cache(maxsize=None)
def _libm():
    m = ctypes.CDLL("libm.so.6")
    for fn in (m.cosf, m.sinf):
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return m


def np_rotation(px, py):
    """{cos(ang), sin(ang), cos(ang2), sin(ang2)} from Python integers and libm's cosf / sinf."""
    m = _libm()
    seed = _py_seed(int(px), int(py))
    out = []
    for s in (seed, seed ^ 0xB5297A4D):
        a = F(F((_py_hash(s) & 0xFFFFFF) / float(1 << 24)) * TWO_PI)
        out += [m.cosf(float(a)), m.sinf(float(a))]
    return np.array(out, F)


def test_rotation_equals_python_and_libm():
    L = soft_lib()
    got, ang = np.zeros(4, F), np.zeros(2, F)
    for px, py in [(0, 0), (5, 7), (799, 599), (3, 500000), (-5, -9)]:
        L.rcs_rotation(px, py, got.ctypes.data, ang.ctypes.data)
        assert np.array_equal(got.view(np.uint32), np_rotation(px, py).view(np.uint32)), (px, py)
        assert 0.0 <= ang[0] < 6.2832 and 0.0 <= ang[1] < 6.2832 and ang[0] != ang[1]


# ---- the sample entry against numpy -------------------------------------------------------------------------------

POISSON = np.array([
    (-0.613392, 0.617481), (0.170019, -0.040254), (-0.299417, 0.791925), (0.645680, 0.493210), (-0.651784, 0.717887),
    (0.421003, 0.027070), (-0.817194, -0.271096), (-0.705374, -0.668203), (0.977050, -0.108615), (0.063326, 0.142369),
    (0.203528, 0.214331), (-0.667531, 0.326090), (-0.098422, -0.295755), (-0.885922, 0.215369), (0.566637, 0.605213),
    (0.039766, -0.396100), (0.751946, 0.453352), (0.078707, -0.715323), (-0.075838, -0.529344), (0.724479, -0.580798),
    (0.222999, -0.215125), (-0.467574, -0.405438), (-0.248268, -0.814753), (0.354411, -0.887570), (0.175817, 0.382366),
    (0.487472, -0.063082), (-0.084078, 0.898312), (0.488876, -0.783441), (0.470016, 0.217933), (-0.696890, -0.549791),
    (-0.149693, 0.605762), (0.034211, 0.979980)], F)


def _np_lround(x):
    """(int)lroundf of a float32 array that is NaN or >= 0: halves away from zero, NaN -> 0."""
    x64 = np.where(np.isnan(x), 0.0, x.astype(np.float64))
    return np.floor(x64 + 0.5).astype(np.int64)


def np_pcss(sm, uv, z, bias, pxpy, k):
    """pcss_shadow_factor (:333-445) over n samples at once, one float32 rounding per operation."""
    sm = np.asarray(sm, F)
    h, w = sm.shape
    u, v = np.asarray(uv, F).reshape(-1, 2).T
    z, bias = np.asarray(z, F), np.asarray(bias, F)
    rot = np.array([np_rotation(px, py) for px, py in np.asarray(pxpy).reshape(-1, 2)], F)

    def outside(a, b):
        return (a < 0) | (a > 1) | (b < 0) | (b > 1)

    def tap(a, b):
        x = np.clip(_np_lround(a * F(w - 1)), 0, w - 1)
        y = np.clip(_np_lround(b * F(h - 1)), 0, h - 1)
        return np.where(outside(a, b), F(FLT_MAX), sm[y, x])
    with np.errstate(all="ignore"):
        early = outside(u, v) | (tap(u, v) == F(FLT_MAX))
        tsu, tsv = F(1) / F(w), F(1) / F(h)
        sru, srv = F(k.search_radius_texels) * tsu, F(k.search_radius_texels) * tsv
        ztest = z - bias
        bsum, bcnt = np.zeros_like(z), np.zeros(z.shape, np.int64)
        for i in range(k.blocker_samples):
            ox = rot[:, 0] * POISSON[i & 31, 0] - rot[:, 1] * POISSON[i & 31, 1]
            oy = rot[:, 1] * POISSON[i & 31, 0] + rot[:, 0] * POISSON[i & 31, 1]
            d = tap(u + ox * sru, v + oy * srv)
            blocks = (d != F(FLT_MAX)) & (d < ztest)
            bsum = np.where(blocks, bsum + d, bsum)
            bcnt += blocks
        avg = bsum / bcnt.astype(F)
        eps = F(k.epsilon)
        zb, zr = np.where(eps < avg, avg, eps), np.where(eps < z, z, eps)
        ratio = (zr - zb) / zb
        ratio = np.where(F(0) < ratio, ratio, F(0))
        fu = F(k.light_uv_radius) * ratio
        ft = F(0.5) * (fu / tsu + fu / tsv)
        lo, hi = F(k.min_filter_texels), F(k.max_filter_texels)
        ft = np.where(ft < lo, lo, np.where(ft > hi, hi, ft))
        fru, frv = ft * tsu, ft * tsv
        lit = np.zeros_like(z)
        for i in range(k.pcf_samples):
            ox = rot[:, 2] * POISSON[i & 31, 0] - rot[:, 3] * POISSON[i & 31, 1]
            oy = rot[:, 3] * POISSON[i & 31, 0] + rot[:, 2] * POISSON[i & 31, 1]
            d = tap(u + ox * fru, v + oy * frv)
            lit = lit + np.where((d == F(FLT_MAX)) | (z <= d + bias), F(1), F(0))
        res = lit / F(k.pcf_samples) if k.pcf_samples > 0 else np.ones_like(z)
    assert all(a.dtype == F for a in (avg, ratio, ft, fru, lit, res))
    return np.where(early | (bcnt <= 0), F(1), res).astype(F), bcnt, ft


@pytest.mark.parametrize("pcss", [None, WIDE, dict(blocker_samples=40, pcf_samples=33, light_uv_radius=0.02)], ids=["demo", "wide", "wrap"])
def test_samples_equal_numpy_restatement(pcss):
    k = demo_pcss(**(pcss or {}))
    sm, uv, z, bias, pxpy = random_samples()
    got, blockers, radius, flags = ref_pcss_samples(sm, uv, z, bias, pxpy, k)
    want, bcnt, ft = np_pcss(sm, uv, z, bias, pxpy, k)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    searched = blockers >= 0
    assert np.array_equal(blockers[searched], bcnt[searched])
    filtered = radius >= 0
    assert np.array_equal(radius[filtered].view(np.uint32), ft[filtered].view(np.uint32))
    # the set meets every branch: early outs, no blocker, partial factors, taps off the map and on empty texels
    for bit in (UV_OUTSIDE, EMPTY_CENTRE, NO_BLOCKER, BLOCKER_OFF_MAP, BLOCKER_EMPTY, PCF_OFF_MAP, PCF_EMPTY):
        assert ((flags & bit) != 0).sum() >= 20, bit
    assert ((got > 0) & (got < 1)).sum() > 500


# ---- known answers ------------------------------------------------------------------------------------------------

def test_pcss_known_answers():
    for name, sm, k, uv, z, bias, pxpy, want, bits in known_cases():
        got, blockers, radius, flags = ref_pcss_samples(sm, [uv], [z], [bias], [pxpy], k)
        if want is not None:
            assert got[0] == want, (name, got[0])
            assert flags[0] & (UV_OUTSIDE | EMPTY_CENTRE | NO_BLOCKER) == bits, (name, flags[0])
        npv, _, _ = np_pcss(sm, [uv], [z], [bias], [pxpy], demo_pcss() if k is None else k)
        assert got[0] == npv[0], name
        if name == "nearer":           # 12 blockers at 0.2: ratio 2, 0.0035 * 2 * 64 = 0.448 texels -> the min clamp
            assert blockers[0] == 12 and radius[0] == 1.0 and flags[0] == 0
        if name == "farther":
            assert blockers[0] == 0 and radius[0] == -1.0
        if name == "no-pcf-samples":
            assert blockers[0] == 12 and radius[0] == 1.0
        if name.startswith("corner-uv"):
            assert flags[0] & BLOCKER_OFF_MAP and flags[0] & PCF_OFF_MAP and 0.0 <= got[0] <= 1.0
        if name == "nan-u-only":
            assert blockers[0] >= 0 and flags[0] & BLOCKER_OFF_MAP and not flags[0] & (UV_OUTSIDE | EMPTY_CENTRE)
        if name == "nan-uv-texel0-blocks":
            assert blockers[0] == 12 and not flags[0] & (BLOCKER_OFF_MAP | BLOCKER_EMPTY | PCF_OFF_MAP | PCF_EMPTY)


def test_sample_counts_above_32_wrap():
    """40 samples are the 32 offsets plus the first 8 again, in the blocker search and in the PCF."""
    sm, uv, z, bias, pxpy = wrap_samples()
    f = {}
    for nb, nt in ((40, 40), (32, 32), (8, 8), (40, 32), (40, 8)):
        f[nb, nt] = ref_pcss_samples(sm, uv, z, bias, pxpy, demo_pcss(blocker_samples=nb, pcf_samples=nt, light_uv_radius=0.03))
    assert np.array_equal(f[40, 40][1], f[32, 32][1] + f[8, 8][1])                  # blocker counts add up
    assert (f[8, 8][1] > 0).sum() > 100 and (f[8, 8][1] < 8).sum() > 100
    # with the same 40 blockers (the same radius) the lit counts of 32 and of 8 taps add up to that of 40
    lit = {nt: np.rint(f[40, nt][0] * F(nt)).astype(int) for nt in (40, 32, 8)}
    on = f[40, 40][1] > 0
    assert on.sum() > 200 and np.array_equal(lit[40][on], lit[32][on] + lit[8][on])
    assert ((lit[8][on] > 0) & (lit[8][on] < 8)).sum() > 50


def test_non_square_map_keeps_the_texel_sizes_apart():
    """96 x 50: one blocker tap, every texel a distinct depth nearer than the receiver.  The tap's texel is the
    centre displaced by (ox * 18 / 96, oy * 18 / 50) in uv -- the two axes' offsets in the ratio of the texel sizes
    -- and the radius that comes out is the one of that texel's depth, with 96 and 50 kept apart in it too."""
    L = soft_lib()
    w, h = 96, 50
    sm = (F(0.1) + np.arange(w * h, dtype=F).reshape(h, w) * F(1e-5)).astype(F)
    k = demo_pcss(blocker_samples=1, pcf_samples=4, light_uv_radius=0.01)
    o = np.zeros(2, F)
    seen = set()
    for px, py in [(1, 2), (30, 4), (77, 55), (120, 9), (15, 110)]:
        L.rcs_rotated_tap(px, py, 0, 0, o.ctypes.data)
        su = F(F(0.5) + F(o[0] * F(F(18) * F(F(1) / F(w)))))
        sv = F(F(0.5) + F(o[1] * F(F(18) * F(F(1) / F(h)))))
        x, y = int(_np_lround(np.array([su * F(w - 1)], F))[0]), int(_np_lround(np.array([sv * F(h - 1)], F))[0])
        dx, dy = x - 0.5 * (w - 1), y - 0.5 * (h - 1)
        assert abs(dx - o[0] * 18 * (w - 1) / w) <= 0.51 and abs(dy - o[1] * 18 * (h - 1) / h) <= 0.51
        d = sm[y, x]
        ratio = F(F(F(0.9) - d) / d)
        fu = F(F(0.01) * ratio)
        want = F(F(0.5) * F(F(fu / F(F(1) / F(w))) + F(fu / F(F(1) / F(h)))))
        got, blockers, radius, _ = ref_pcss_samples(sm, [(0.5, 0.5)], [0.9], [0.0], [(px, py)], k)
        assert blockers[0] == 1 and radius[0] == want and 1.0 < want < 28.0, (px, py, radius[0], want)
        seen.add((x, y))
    assert len(seen) == 5 and any(abs(x - 47.5) > 6 for x, _ in seen) and any(abs(y - 24.5) > 6 for _, y in seen)


# ---- the camera pass ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["demo", "near", "coincident"])
def test_without_a_map_the_raster_is_the_hard_demos(name):
    """The raster is the same: depth, sub-triangle ids and counters equal test_canvas_rt_ref's.  The colours differ
    by the shader's constants: ambient 0.22 * base for 0.18 * base, and the specular term (0.45 * spec) added after
    the diffuse term took the base colour, not multiplied by it.  No velocity."""
    view, lvp, draws = R.SCENES[name]()
    hard = R.ref_render(R._frame(view, lvp, use_shadow=False), draws)
    soft = ref_render_soft(soft_frame(view, lvp, use_shadow=False), draws)
    helpers.assert_depth_bitexact(soft["depth"], hard["depth"])
    assert np.array_equal(soft["tri_id"], hard["tri_id"]) and soft["counters"] == hard["counters"]
    assert np.array_equal(soft["texel"], hard["texel"])
    assert not soft["velocity"].any()
    shaded = soft["tri_id"] >= 0
    assert shaded.sum() > 1000 and (soft["color"][shaded] != hard["color"][shaded]).any()
    assert (soft["prequant"][..., 3][shaded] == 1.0).all() and (soft["pcss_flags"][shaded] == NOT_IN_LIGHT).all()
    # where the light does not reach (diffuse and specular zero) the two differ by the ambient alone
    dark = shaded & (hard["prequant"][..., 0] > 0) & np.isclose(hard["prequant"][..., 0] * (0.22 / 0.18), soft["prequant"][..., 0], rtol=1e-5)
    assert name != "demo" or dark.sum() > 20


@functools.lru_cache(maxsize=None)
def soft_planes(name, wide=False, sm=SM, tile=80, casters_from=0):
    """(shadow map, soft planes) of a scene; casters_from = 1 leaves the first draw (the floor) out of PASS0, so its
    fragments find an empty centre texel or empty texels around the objects' shadows."""
    view, lvp, draws = R.SCENES[name]()
    shadow = R.ref_shadow(sm, lvp, draws[casters_from:], (tile, tile))
    return shadow, ref_render_soft(soft_frame(view, lvp, tile=(tile, tile)), draws, shadow, demo_pcss(**WIDE) if wide else None)


def _count(out, bit):
    return int(((out["pcss_flags"] & bit) != 0).sum())


def _seen(out, hi):
    shaded = out["tri_id"] >= 0
    fac, rad = out["prequant"][..., 3], out["radius"]
    filtered = shaded & (rad >= 0)
    return {
        "partial": int((shaded & (fac > 0) & (fac < 1)).sum()), "dark": int((shaded & (fac == 0)).sum()),
        "min": int((filtered & (rad == 1.0)).sum()), "between": int((filtered & (rad > 1.0) & (rad < hi)).sum()),
        "max": int((filtered & (rad == hi)).sum()), "no_blocker": _count(out, NO_BLOCKER),
        "blocker_off": _count(out, BLOCKER_OFF_MAP), "blocker_empty": _count(out, BLOCKER_EMPTY),
        "pcf_off": _count(out, PCF_OFF_MAP), "pcf_empty": _count(out, PCF_EMPTY), "uv_outside": _count(out, UV_OUTSIDE),
        "empty_centre": _count(out, EMPTY_CENTRE), "not_in_light": _count(out, NOT_IN_LIGHT),
    }


# Minimum pixel counts per scene; beside each, in the comment, what the restatement shows (x86-64, glibc).
NEED = {
    # the miniature, widened constants: factors strictly inside (0, 1); radii at the min clamp, between the clamps and
    # at the max clamp; no blocker under a non-empty centre; blocker taps off the map and on empty texels; PCF taps off
    # the map.   partial 12158, dark 91, min 525, between 10464, max 1734, no_blocker 742, blocker_off 2865,
    # blocker_empty 91, pcf_off 43, uv_outside 617
    "demo-wide": dict(partial=6000, dark=40, min=250, between=5000, max=800, no_blocker=350, blocker_off=1400, blocker_empty=40,
                      pcf_off=20, uv_outside=300),
    # the floor left out of PASS0: empty centre texels and PCF taps on empty texels.
    # empty_centre 11770, pcf_empty 458, blocker_empty 1695, partial 770, min 180, between 554, max 190
    "demo-wide-objects": dict(empty_centre=5000, pcf_empty=200, blocker_empty=800, partial=350, min=90, between=250, max=90),
    # the small light box: receivers outside its depth range and extent, PCF taps off the map and on empty texels.
    # not_in_light 6004, uv_outside 6572, pcf_off 47, pcf_empty 95, blocker_off 504, blocker_empty 434, max 1167
    "outside-wide": dict(not_in_light=3000, uv_outside=3000, pcf_off=20, pcf_empty=40, blocker_off=250, blocker_empty=200, max=500),
    # 96 x 50.   partial 12692, min 645, between 8992, max 3332, blocker_off 7572
    "demo-wide-96x50": dict(partial=6000, min=300, between=4000, max=1500, blocker_off=3500),
}


def test_scenes_cover_what_the_gpu_tests_need():
    hi = WIDE["max_filter_texels"]
    for key, planes in (("demo-wide", soft_planes("demo", wide=True)), ("demo-wide-objects", soft_planes("demo", wide=True, casters_from=1)),
                        ("outside-wide", soft_planes("outside", wide=True)), ("demo-wide-96x50", soft_planes("demo", wide=True, sm=(96, 50)))):
        seen = _seen(planes[1], hi)
        print(key, seen)
        assert all(seen[k] >= v for k, v in NEED[key].items()), (key, seen)
        assert not planes[1]["velocity"].any()
    assert (soft_planes("demo", wide=True)[1]["texel"] >= 0).sum() > 200
    # the demo's constants: at 96 texels every radius sits at the min clamp (0.0035 * ratio * 96 < 1 while ratio < 3)
    seen = _seen(soft_planes("demo")[1], 28.0)
    print("demo", seen)
    assert seen["min"] > 6000 and seen["between"] == 0 and seen["max"] == 0 and seen["partial"] > 3000      # min 12704, partial 7653
