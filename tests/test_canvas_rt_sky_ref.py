"""tests/canvas_rt_sky_ref (ref_canvas_rt_sky.c), the C restatement of skybox_background_pass and of the legacy
AnalyticSky / CubeMapSky (hello-shs-renderer/shs_renderer.hpp) -- the reference of tests/test_canvas_rt_sky.py -- pinned
on the CPU:

  * against a second restatement in float32 numpy, written from the same cited lines, bit for bit: both sample
    functions on seeded random and edge directions, the per-pixel direction and the linear radiance of whole frames.
    The three std::pow of AnalyticSky and the sRGB table go through libm's powf, the function the C file calls (numpy's
    float32 power is another implementation), and those powf values are compared against float64 x ** n within one
    float32 ulp; the encoded bytes go under the parity rule of helpers.assert_color_parity;
  * by known answers of both models;
  * with the ABI struct's size and offsets against the ctypes mirror;
  * and the frames of the GPU test are checked, on the restatement alone, to show what they are there for.

It also holds what fails without the feature and needs no GPU: the new entry points and the struct."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import helpers
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
from test_canvas_rt_ref import F, H, W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_rt_sky_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_rt_sky_ref.so")
_P = ctypes.c_void_p
_F3 = ctypes.c_float * 3
ANALYTIC, CUBEMAP = 1, 2
REINHARD, CLAMP = 0, 1
BRANCH_NONE, BRANCH_EDGE, BRANCH_DISC = 0, 1, 2
DISC = np.array([4.0, 3.5, 3.0], F)


class RefFace(ctypes.Structure):
    _fields_ = [("rgba", _P), ("w", ctypes.c_int32), ("h", ctypes.c_int32)]


class RefSky(ctypes.Structure):
    _fields_ = [("model", ctypes.c_int32), ("encode", ctypes.c_int32), ("sun_dir", _F3), ("intensity", ctypes.c_float),
                ("face", RefFace * 6), ("cam_forward", _F3), ("cam_right", _F3), ("cam_up", _F3), ("fov_degrees", ctypes.c_float),
                ("exposure", ctypes.c_float)]


@functools.lru_cache(maxsize=None)
def sky_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    L = ctypes.CDLL(REF_LIB)
    L.rsk_compose.restype = ctypes.c_int
    L.rsk_compose.argtypes = [ctypes.POINTER(RefSky), ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P, _P]
    L.rsk_samples.restype = ctypes.c_int
    L.rsk_samples.argtypes = [ctypes.POINTER(RefSky), ctypes.c_int, _P, _P, _P]
    L.rsk_render_pbr.restype = ctypes.c_int
    L.rsk_render_pbr.argtypes = [ctypes.POINTER(RefSky), ctypes.POINTER(R.RefFrame), ctypes.POINTER(P.RefConsts), ctypes.POINTER(P.RefIbl),
                                 ctypes.POINTER(R.RefDraw), ctypes.POINTER(P.RefMaterial), ctypes.c_int, ctypes.POINTER(R.RefPlanes),
                                 ctypes.POINTER(P.RefDebugPlanes)]
    L.rsk_sizeof_sky.restype = ctypes.c_size_t
    L.rsk_sizeof_sky.argtypes = []
    return L


# ---- the skies, the cameras and the frames (shared with tests/test_canvas_rt_sky.py) ------------------------

class Tex:
    """An object with .rgba [h, w, 4], what shs_gpu.Context.upload_texture takes."""

    def __init__(self, rgba):
        self.rgba = np.ascontiguousarray(rgba, np.uint8)


# (w, h) of +X -X +Y -Y +Z -Z: all different, one square, one 1 x 1, none a multiple of another's both sides
FACE_SIZES = ((4, 4), (5, 3), (1, 1), (7, 2), (2, 6), (3, 8))
ODD_SIZES = ((3, 3), (5, 3), (1, 1), (7, 5), (3, 9), (5, 5))   # every face has a centre texel


@functools.lru_cache(maxsize=None)
def make_faces(seed=5, sizes=FACE_SIZES):
    rng = np.random.default_rng(seed)
    return tuple(Tex(rng.integers(0, 256, (h, w, 4))) for w, h in sizes)


def normalized(v):
    v = np.asarray(v, np.float64)
    return tuple(float(x) for x in v / np.linalg.norm(v))


def camera_vectors(forward, world_up=(0.0, 1.0, 0.0)):
    """Camera3D's direction, right and up vectors of a camera looking along forward (any lengths would do: the pass
    normalises them)."""
    f = np.asarray(normalized(forward))
    r = np.cross(np.asarray(world_up, np.float64), f)
    r = r / np.linalg.norm(r)
    u = np.cross(f, r)
    return dict(cam_forward=tuple(f), cam_right=tuple(r), cam_up=tuple(u))


def camera_of_view(view):
    """The vectors of the camera test_canvas_rt_ref.camera() looks through: lookAtLH's s, u and f rows."""
    m = np.asarray(view, F).reshape(4, 4)   # m[c][r]
    return dict(cam_right=tuple(float(v) for v in m[:3, 0]), cam_up=tuple(float(v) for v in m[:3, 1]),
                cam_forward=tuple(float(v) for v in m[:3, 2]))


def elevated(deg, azimuth_deg=0.0):
    e, a = np.radians(deg), np.radians(azimuth_deg)
    return (float(np.cos(e) * np.sin(a)), float(np.sin(e)), float(np.cos(e) * np.cos(a)))


def analytic_sky(sun_at, encode=REINHARD, **cam):
    """AnalyticSky whose sun stands in direction sun_at (sun_direction points away from it)."""
    import shs_gpu
    return shs_gpu.RtSky(model=ANALYTIC, encode=encode, sun_dir=tuple(-v for v in sun_at), **cam)


def cubemap_sky(faces=None, intensity=1.0, encode=CLAMP, **cam):
    import shs_gpu
    return shs_gpu.RtSky(model=CUBEMAP, encode=encode, intensity=intensity, face_tex=tuple(make_faces() if faces is None else faces), **cam)


SUN_UP = elevated(10.0)                   # 10 degrees over the horizon, straight ahead (+z)
SUN_DOWN = (0.6, -0.3, 0.74)              # below the horizon: sun_height = 0
# The analytic frames: the sun at the view centre -- its disc, the ring around it and, over the 60 degrees of the view, rows
# above cosTheta 0.15, inside the band and below it -- and a second camera pitched down at the ground.
AT_SUN = dict(fov_degrees=60.0, **camera_vectors(SUN_UP))
PITCHED_DOWN = dict(fov_degrees=60.0, **camera_vectors(elevated(-35.0, 20.0)))
# The cubemap frames: two wide cameras back to back, which together see all six faces.
WIDE_A = dict(fov_degrees=140.0, **camera_vectors((1.0, 0.8, 0.6)))
WIDE_B = dict(fov_degrees=140.0, **camera_vectors((-1.0, -0.8, -0.6)))


def frame_skies():
    """(name, RtSky) of the whole-frame tests: each model under each encode."""
    return [
        ("analytic-reinhard", analytic_sky(SUN_UP, REINHARD, **AT_SUN)),
        ("analytic-clamp", analytic_sky(SUN_UP, CLAMP, **AT_SUN)),
        ("analytic-down", analytic_sky(SUN_UP, REINHARD, **PITCHED_DOWN)),
        ("cubemap-clamp", cubemap_sky(intensity=1.0, encode=CLAMP, **WIDE_A)),
        ("cubemap-reinhard", cubemap_sky(intensity=2.5, encode=REINHARD, **WIDE_B)),
    ]


def demo_skies():
    """The skies of the demo in miniature, through test_canvas_rt_ref's camera: hello_pbr.cpp's analytic sky with the sun
    low over the far end of the floor, and a cubemap."""
    view, _ = R.camera()
    cam = dict(fov_degrees=60.0, **camera_of_view(view))
    return [("analytic", analytic_sky(elevated(5.0), REINHARD, **cam)), ("cubemap", cubemap_sky(intensity=1.5, encode=REINHARD, **cam))]


def _sky_c(sky, keep):
    s = RefSky()
    s.model, s.encode = int(sky.model), int(sky.encode)
    s.intensity, s.fov_degrees, s.exposure = float(sky.intensity), float(sky.fov_degrees), float(sky.exposure)
    for name in ("sun_dir", "cam_forward", "cam_right", "cam_up"):
        getattr(s, name)[:] = [float(v) for v in getattr(sky, name)]
    for k, t in enumerate(sky.face_tex):
        rgba = np.ascontiguousarray(t.rgba, np.uint8)
        keep.append(rgba)
        s.face[k].rgba, s.face[k].w, s.face[k].h = rgba.ctypes.data, rgba.shape[1], rgba.shape[0]
    return s


def ref_samples(sky, dirs):
    """sky.sample(dir) -> (radiance [n, 3], debug [n, 2]: analytic (branch, band), cubemap (face or -1, 0))"""
    keep = []
    s = _sky_c(sky, keep)
    dirs = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    out, dbg = np.empty_like(dirs), np.empty((dirs.shape[0], 2), np.int32)
    assert sky_lib().rsk_samples(ctypes.byref(s), dirs.shape[0], dirs.ctypes.data, out.ctypes.data, dbg.ctypes.data) == 0
    return out, dbg


def ref_compose(sky, planes, w=None, h=None):
    """The background under a rendered frame's planes (a dict with 'color', 'prequant', 'tri_id'; None: the pass alone
    over w x h) -> a copy with the sky where tri_id < 0, plus 'sky_dir' [.., 3], 'sky_lin' [.., 3], 'sky_dbg' [.., 2]
    (zeros / -9 where a fragment is shown)."""
    if planes is None:
        planes = {"color": np.zeros((h, w, 4), np.uint8), "prequant": np.zeros((h, w, 4), F), "tri_id": np.full((h, w), -1, np.int32)}
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in planes.items()}
    hh, ww = out["tri_id"].shape
    out.update(sky_dir=np.zeros((hh, ww, 3), F), sky_lin=np.zeros((hh, ww, 3), F), sky_dbg=np.full((hh, ww, 2), -9, np.int32))
    keep = []
    s = _sky_c(sky, keep)
    assert sky_lib().rsk_compose(ctypes.byref(s), ww, hh, out["tri_id"].ctypes.data, out["color"].ctypes.data, out["prequant"].ctypes.data,
                                 out["sky_dir"].ctypes.data, out["sky_lin"].ctypes.data, out["sky_dbg"].ctypes.data) == 0
    return out


def ref_render_pbr_sky(sky, frame, draws, mats, shadow=None, ibl=None, consts=None):
    """hello_pbr.cpp's PASS1 with its background in one call of the C file (rsk_render_pbr): the planes of
    test_canvas_rt_pbr_ref.ref_render_pbr without the debug planes."""
    Wd, Hd = frame.width, frame.height
    keep = []
    arr = R._ref_draws(draws, keep)
    f = P._frame_c(frame, shadow, keep)
    out = {"color": np.empty((Hd, Wd, 4), np.uint8), "depth": np.empty((Hd, Wd), F), "velocity": np.empty((Hd, Wd, 2), F),
           "prequant": np.empty((Hd, Wd, 4), F), "tri_id": np.empty((Hd, Wd), np.int32)}
    p = R.RefPlanes()
    for k, v in out.items():
        setattr(p, k, v.ctypes.data)
    kc, ic, s = P._consts_c(consts), P._ibl_c(ibl, keep), _sky_c(sky, keep)
    assert sky_lib().rsk_render_pbr(ctypes.byref(s), ctypes.byref(f), ctypes.byref(kc), None if ic is None else ctypes.byref(ic), arr,
                                    P._materials_c(mats), len(draws), ctypes.byref(p), None) == 0
    return out


# ---- sample sets (shared with the GPU test) -------------------------------------------------------------------

def random_directions(seed=41, n=4096):
    """n directions of every length and sign; some on the cube's ties, a good many within two degrees of the sun of
    SUN_UP (the glow, the ring and the disc) and on the horizon band's two edges."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)).astype(F) * rng.choice(np.array([1e-3, 1.0, 50.0], F), size=(n, 1))
    d[::64] = np.sign(d[::64]) * F(0.75)                       # |x| == |y| == |z|: the tie order decides
    d[1::64, 1] = d[1::64, 0]                                  # |x| == |y|
    d[2::64, 2] = -d[2::64, 1]                                 # |y| == |z|
    near = (np.asarray(SUN_UP)[None, :] + rng.normal(size=(len(d[3::8]), 3)) * 0.02) * rng.uniform(0.5, 3.0, (len(d[3::8]), 1))
    d[3::8] = near.astype(F)
    band = rng.normal(size=(len(d[5::16]), 3))
    band[:, 1] = np.sign(band[:, 1]) * 0.15 * np.sqrt((band[:, 0] ** 2 + band[:, 2] ** 2) / (1 - 0.15 ** 2)) * rng.uniform(0.98, 1.02, len(band))
    d[5::16] = band.astype(F)
    return d


def edge_directions():
    """(name, direction): what the issue lists, for both models."""
    c = float(np.sqrt(1.0 - 0.15 ** 2))
    return [("up", (0, 1, 0)), ("down", (0, -1, 0)), ("horizon+0.15", (c, 0.15, 0)), ("horizon-0.15", (0, -0.15, c)), ("along-s", SUN_UP),
            ("along-s-long", tuple(7.0 * v for v in SUN_UP)), ("zero", (0, 0, 0)), ("tiny", (1e-9, -1e-9, 1e-9)),
            ("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+y", (0, 2, 0)), ("-y", (0, -2, 0)), ("+z", (0, 0, 3)), ("-z", (0, 0, -3)),
            ("edge-xy", (1, 1, 0)), ("edge-yz", (0, 1, -1)), ("edge-xz", (-1, 0, 1)), ("corner+", (2, 2, 2)), ("corner-", (-2, -2, -2)),
            ("corner-mixed", (1, -1, 1))]


def nan_directions():
    nan, inf = float("nan"), float("inf")
    return np.array([(nan, 0, 0), (0, nan, 1), (1, 2, nan), (nan, nan, nan), (inf, 0, 0), (1, -inf, 1)], F)


# ---- what fails without the feature, without a GPU ---------------------------------------------------------

NEW_ENTRY_POINTS = ("shs_rt_set_sky", "shs_rt_sky_samples")


def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in NEW_ENTRY_POINTS + ("shs_rt_render", "shs_rt_render_pbr"):
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_ctypes_sky_struct_has_the_headers_layout(tmp_path):
    """sizeof and every member's offset of shs_rt_sky against the ctypes mirror; shs_rt_frame, shs_rt_draw and
    shs_rt_pbr_draw keep their sizes."""
    from shs_gpu import _abi
    names = [n for n, _ in _abi.RtSkyC._fields_]
    offs = ", ".join(f"offsetof(shs_rt_sky, {n})" for n in names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shs_gpu.h"\nint main(void) {\n'
                   f'    size_t v[] = {{sizeof(shs_rt_sky), {offs}, sizeof(shs_rt_frame), sizeof(shs_rt_draw), sizeof(shs_rt_pbr_draw)}};\n'
                   '    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]);\n'
                   f'    printf("%d %d %d %d %d\\n", SHS_RT_SKY_NONE, SHS_RT_SKY_ANALYTIC, SHS_RT_SKY_CUBEMAP, SHS_RT_SKY_ENCODE_REINHARD, '
                   'SHS_RT_SKY_ENCODE_CLAMP);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_abi.RtSkyC)] + [getattr(_abi.RtSkyC, n).offset for n in names]
    assert got[:len(want)] == want and got[0] == 92
    assert got[len(want):len(want) + 3] == [ctypes.sizeof(_abi.RtFrameC), ctypes.sizeof(_abi.RtDrawC), ctypes.sizeof(_abi.RtPbrDrawC)] == [192, 204, 60]
    assert got[-5:] == [_abi.RT_SKY_NONE, _abi.RT_SKY_ANALYTIC, _abi.RT_SKY_CUBEMAP, _abi.RT_SKY_ENCODE_REINHARD, _abi.RT_SKY_ENCODE_CLAMP]
    assert (ANALYTIC, CUBEMAP, REINHARD, CLAMP) == (_abi.RT_SKY_ANALYTIC, _abi.RT_SKY_CUBEMAP, _abi.RT_SKY_ENCODE_REINHARD, _abi.RT_SKY_ENCODE_CLAMP)
    # the restatement's struct differs in the faces alone (a pointer and two ints each instead of an id)
    assert sky_lib().rsk_sizeof_sky() == ctypes.sizeof(RefSky)


# ---- the second restatement: float32 numpy -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _libm():
    m = ctypes.CDLL("libm.so.6")
    m.powf.restype = ctypes.c_float
    m.powf.argtypes = [ctypes.c_float, ctypes.c_float]
    m.tanf.restype = ctypes.c_float
    m.tanf.argtypes = [ctypes.c_float]
    return m


def _powf(x, n):
    """libm's powf over an array, the function the C restatement calls"""
    x = np.asarray(x, F)
    p = _libm().powf
    return np.array([p(float(v), float(n)) for v in x.ravel()], F).reshape(x.shape)


def _gmin(x, y):
    return np.where(y < x, y, x).astype(F)   # glm::min(x, y): (y < x) ? y : x


def _gmax(x, y):
    return np.where(x < y, y, x).astype(F)   # glm::max(x, y): (x < y) ? y : x


def _clamp(x, lo, hi):
    return _gmin(_gmax(x, F(lo)), F(hi))


def _mix(x, y, a):
    a = np.asarray(a, F)   # glm::mix(x, y, a): x * (1 - a) + y * a
    return (x * (F(1) - a) + y * a).astype(F)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    v = np.asarray(v, F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (v * (F(1) / np.sqrt(_dot(v, v)))[..., None]).astype(F)


def np_analytic(sun_direction, dirs):
    """AnalyticSky::sample (shs_renderer.hpp:558-608) over dirs [n, 3] -> (radiance [n, 3], branch [n], band [n], the
    three pow arguments [3, n], the colour before the disc / ring branches [n, 3])"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = _normalize(dirs)
        s = -_normalize(np.asarray(sun_direction, F))
        cos_theta = _clamp(d[:, 1], -1, 1)
        cos_gamma = _dot(d, s[None, :])
        v3 = lambda *c: np.array(c, F)   # noqa: E731
        sun_height = _clamp(s[1], 0, 1)
        zenith = _mix(v3(0.02, 0.02, 0.05), v3(0.30, 0.70, 1.70), sun_height)
        horizon = _mix(v3(0.4, 0.15, 0.05), v3(1.30, 1.64, 2.00), sun_height)
        base = v3(0.30, 0.26, 0.22)
        ground = _mix(base * F(0.5), base, sun_height)
        ground = ground + horizon * F(0.05)
        tmp = _clamp((cos_theta - F(-0.15)) / (F(0.15) - F(-0.15)), 0, 1)
        factor = tmp * tmp * (F(3) - F(2) * tmp)
        args = np.stack([F(1) - _gmax(F(0), cos_theta), F(1) + _gmin(F(0), cos_theta), _clamp(cos_gamma, 0, 1)]).astype(F)
        upper = _mix(zenith[None, :], horizon[None, :], _powf(args[0], 3.0)[:, None])
        lower = _mix(ground[None, :], (horizon * F(0.5))[None, :], _powf(args[1], 4.0)[:, None])
        sky = _mix(lower, upper, factor[:, None])
        glow = (v3(1.0, 0.8, 0.4) * F(4)) * sun_height
        sky = sky + glow[None, :] * _powf(args[2], 12.0)[:, None]
        before = sky.astype(F)
        disc = cos_gamma > F(0.9998)
        ring = ~disc & (cos_gamma > F(0.9992))
        edge = (cos_gamma - F(0.9992)) / (F(0.9998) - F(0.9992))
        sky = np.where(ring[:, None], _mix(sky, v3(3.0, 2.5, 1.5)[None, :], edge[:, None]), sky)
        sky = np.where(disc[:, None], DISC[None, :], sky).astype(F)
        band = np.where(cos_theta > F(0.15), 2, np.where(cos_theta < F(-0.15), 0, 1))
    return sky, np.where(disc, BRANCH_DISC, np.where(ring, BRANCH_EDGE, BRANCH_NONE)), band, args, before


def np_cubemap(faces, intensity, dirs):
    """CubeMapSky::sample over sample_face_bilinear (shs_renderer.hpp:439-512) -> (radiance [n, 3], face [n], -1: zero length)"""
    lut = P._powf_table()
    d = np.asarray(dirs, F)
    n = d.shape[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ln = np.sqrt(_dot(d, d))
        zero = ln < F(1e-8)
        d = (d / ln[:, None]).astype(F)
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        cx = (ax >= ay) & (ax >= az)
        cy = ~cx & (ay >= ax) & (ay >= az)
        face = np.where(cx, np.where(x > 0, 0, 1), np.where(cy, np.where(y > 0, 2, 3), np.where(z > 0, 4, 5)))
        u = np.choose(face, [-z / ax, z / ax, x / ay, x / ay, x / az, -x / az])
        v = np.choose(face, [y / ax, y / ax, -z / ay, z / ay, y / az, y / az])
        u, v = _clamp(F(0.5) * (u + F(1)), 0, 1), _clamp(F(0.5) * (v + F(1)), 0, 1)
        out = np.zeros((n, 3), F)
        for f in range(6):
            pick = (face == f) & ~zero
            if not pick.any():
                continue
            rgba = np.asarray(faces[f].rgba, np.uint8)
            h, w = rgba.shape[:2]
            fx, fy = u[pick] * F(w - 1), v[pick] * F(h - 1)
            INT_MIN = -2 ** 31
            x0 = np.where(np.isnan(fx), INT_MIN, np.floor(np.nan_to_num(fx))).astype(np.int64)   # (int)std::floor on x86-64
            y0 = np.where(np.isnan(fy), INT_MIN, np.floor(np.nan_to_num(fy))).astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
            tx, ty = (fx - x0.astype(F)).astype(F), (fy - y0.astype(F)).astype(F)

            def get(xx, yy):   # Texture2D::get, then to_lin through the table
                inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                t = rgba[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1), :3]
                return lut[np.where(inside[:, None], t, 0)]

            vx0 = _mix(get(x0, y0), get(x1, y0), tx[:, None])
            vx1 = _mix(get(x0, y1), get(x1, y1), tx[:, None])
            out[pick] = _mix(vx0, vx1, ty[:, None]) * F(intensity)
    return out, np.where(zero, -1, face)


def np_sample(sky, dirs):
    if sky.model == CUBEMAP:
        rgb, face = np_cubemap(sky.face_tex, sky.intensity, dirs)
        return rgb, face
    rgb, branch, _, _, _ = np_analytic(sky.sun_dir, dirs)
    return rgb, branch


def np_directions(sky, w, h):
    """The pass's direction of every canvas pixel (hello_pbr.cpp:743-748, :769-780) -> [h, w, 3]"""
    aspect = F(w) / F(h)
    tan_half = F(_libm().tanf(float(F(sky.fov_degrees) * F(0.01745329251994329576923690768489) * F(0.5))))
    fwd, right, up = (_normalize(np.asarray(getattr(sky, n), F)) for n in ("cam_forward", "cam_right", "cam_up"))
    fx = ((np.arange(w, dtype=F) + F(0.5)) / F(w)).astype(F)
    fy = ((np.arange(h, dtype=F) + F(0.5)) / F(h)).astype(F)
    kx = ((fx * F(2) - F(1)) * aspect * tan_half).astype(F)
    ky = ((fy * F(2) - F(1)) * tan_half).astype(F)
    d = (fwd[None, None, :] + right[None, None, :] * kx[None, :, None]) + up[None, None, :] * ky[:, None, None]
    return _normalize(d.astype(F))


def np_encode(sky, lin):
    """-> (r, g, b) * 255 before the truncation (numpy's float32 power for linear_to_srgb)"""
    c = np.asarray(lin, F)
    with np.errstate(invalid="ignore"):
        if sky.encode == CLAMP:
            c = _clamp(c, 0, 1)
        else:
            c = c * F(sky.exposure)
            c = c / (F(1) + c)
        s = np.power(_clamp(c, 0, 1), F(1.0) / F(2.2)).astype(F)
        return (_clamp(s, 0, 1) * F(255)).astype(F)


def test_numpy_samples_equal_the_restatement_bitwise():
    d = np.concatenate([random_directions(), np.array([e[1] for e in edge_directions()], F)])
    for sun in (SUN_UP, SUN_DOWN, elevated(80.0, 200.0)):
        sky = analytic_sky(sun)
        ref, dbg = ref_samples(sky, d)
        fin = np.isfinite(ref).all(-1)                       # (a zero-length direction into AnalyticSky is NaN either way)
        assert fin.sum() > len(d) - 200
        rgb, branch, band, _, _ = np_analytic(sky.sun_dir, d)
        assert np.array_equal(np.isfinite(rgb).all(-1), fin)
        assert np.array_equal(rgb[fin].view(np.uint32), ref[fin].view(np.uint32))
        assert np.array_equal(branch[fin], dbg[fin, 0]) and np.array_equal(band[fin], dbg[fin, 1])
    d = np.concatenate([d, nan_directions()])
    for faces, intensity in ((make_faces(), 1.0), (make_faces(9, ODD_SIZES), 0.37), (make_faces(), 3.0)):
        sky = cubemap_sky(faces, intensity)
        ref, dbg = ref_samples(sky, d)
        rgb, face = np_cubemap(faces, intensity, d)
        assert np.array_equal(P.canonical_bits(rgb), P.canonical_bits(ref)) and np.array_equal(face, dbg[:, 0])
        assert set(dbg[:, 0].tolist()) == set(range(-1, 6))


def test_libm_pows_are_within_an_ulp_of_float64():
    """The three std::pow(x, 3.0f / 4.0f / 12.0f) of AnalyticSky, as the restatement evaluates them (libm's powf), against
    float64 x ** n: within one float32 ulp of it on every argument the sample set produces."""
    _, _, _, args, _ = np_analytic(analytic_sky(SUN_UP).sun_dir, random_directions())
    for x, n in zip(args, (3.0, 4.0, 12.0)):
        x = x[np.isfinite(x)]
        assert len(x) > 3000 and x.min() >= 0 and x.max() <= 1
        want = x.astype(np.float64) ** n
        got = _powf(x, n).astype(np.float64)
        ulp = np.spacing(np.maximum(want, np.finfo(F).tiny).astype(F)).astype(np.float64)
        assert (np.abs(got - want) <= ulp).all(), (n, np.abs(got - want).max())


def test_numpy_frames_equal_the_restatement():
    """Every pixel of the pass alone, 160 x 120 and 161 x 119: the direction and the linear radiance bit for bit, the
    bytes under the parity rule."""
    for name, sky in frame_skies():
        for w, h in ((W, H), (161, 119)):
            ref = ref_compose(sky, None, w, h)
            d = np_directions(sky, w, h)
            assert np.array_equal(d.view(np.uint32), ref["sky_dir"].view(np.uint32)), name
            lin, what = np_sample(sky, d.reshape(-1, 3))
            assert np.array_equal(lin.reshape(h, w, 3).view(np.uint32), ref["sky_lin"].view(np.uint32)), name
            assert np.array_equal(what.reshape(h, w), ref["sky_dbg"][..., 0]), name
            pre = np_encode(sky, lin).reshape(h, w, 3)
            rgba = np.concatenate([pre.astype(np.uint8), np.full((h, w, 1), 255, np.uint8)], axis=-1)
            helpers.assert_color_parity(rgba, ref["color"], pre, ref["prequant"][..., :3])
            assert (ref["prequant"][..., 3] == 1).all() and (ref["color"][..., 3] == 255).all()


# ---- known answers ------------------------------------------------------------------------------------------

def _one(sky, d):
    rgb, dbg = ref_samples(sky, [d])
    return rgb[0], tuple(dbg[0])


def _f64_sky(s, cos_theta, cos_gamma):
    """AnalyticSky away from the disc and the ring, in float64, for the known answers below"""
    mix = lambda x, y, a: np.asarray(x) * (1 - a) + np.asarray(y) * a   # noqa: E731
    sh = min(max(s[1], 0.0), 1.0)
    zen, hor = mix((0.02, 0.02, 0.05), (0.30, 0.70, 1.70), sh), mix((0.4, 0.15, 0.05), (1.30, 1.64, 2.00), sh)
    gb = np.array((0.30, 0.26, 0.22))
    ground = mix(gb * 0.5, gb, sh) + hor * 0.05
    t = min(max((cos_theta + 0.15) / 0.3, 0.0), 1.0)
    upper = mix(zen, hor, (1 - max(0.0, cos_theta)) ** 3)
    lower = mix(ground, hor * 0.5, (1 + min(0.0, cos_theta)) ** 4)
    return mix(lower, upper, t * t * (3 - 2 * t)) + np.array((1.0, 0.8, 0.4)) * 4 * sh * min(max(cos_gamma, 0.0), 1.0) ** 12


def test_analytic_known_answers():
    day, night = analytic_sky(SUN_UP), analytic_sky(SUN_DOWN)
    s_day, s_night = np.asarray(normalized(SUN_UP)), np.asarray(normalized(SUN_DOWN))
    # a sun below the horizon: sun_height = 0, so straight up is the night zenith exactly, and straight down the night
    # ground, each a handful of exact float32 operations; no glow at all
    up, dbg = _one(night, (0, 1, 0))
    assert np.array_equal(up, np.array([0.02, 0.02, 0.05], F)) and dbg == (BRANCH_NONE, 2)
    down, dbg = _one(night, (0, -1, 0))
    want = (np.array([0.30, 0.26, 0.22], F) * F(0.5)) * F(1) + np.array([0.30, 0.26, 0.22], F) * F(0) + np.array([0.4, 0.15, 0.05], F) * F(0.05)
    assert np.array_equal(down, want.astype(F)) and dbg == (BRANCH_NONE, 0)
    # by day: straight up is the mixed zenith plus the glow's s.y ** 12, straight down the mixed ground
    for d, ct in (((0, 1, 0), 1.0), ((0, -1, 0), -1.0)):
        got, dbg = _one(day, d)
        assert np.abs(got - _f64_sky(s_day, ct, ct * s_day[1])).max() < 2e-6 and dbg[0] == BRANCH_NONE
    # the horizon band's edges: at cosTheta = 0.15 the smoothstep has reached the upper sky, at -0.15 the lower one
    c = float(np.sqrt(1.0 - 0.15 ** 2))
    for d in ((c, 0.15, 0), (0, -0.15, c), (-c, 0.15, 0)):
        got, dbg = _one(night, d)
        assert np.abs(got - _f64_sky(s_night, d[1], float(np.dot(d, s_night)))).max() < 2e-6 and dbg[0] == BRANCH_NONE
        half = (0.02, 0.02, 0.05) if d[1] > 0 else (0.15 + 0.02, 0.13 + 0.0075, 0.11 + 0.0025)   # night zenith / ground
        other = np.array((0.4, 0.15, 0.05)) * (1.0 if d[1] > 0 else 0.5)                         # night horizon (halved below)
        w = 0.85 ** 3 if d[1] > 0 else 0.85 ** 4
        assert np.abs(got - (np.array(half) * (1 - w) + other * w)).max() < 2e-6                 # the other half's weight is 0
    # exactly along s, at any length: the disc's colour, whatever the rest computed
    for k in (1.0, 7.0, 1e-3):
        got, dbg = _one(day, tuple(k * v for v in SUN_UP))
        assert np.array_equal(got, DISC) and dbg[0] == BRANCH_DISC
    # the ring: 1.5 degrees off the sun is between the two thresholds and ends between the sky and (3, 2.5, 1.5)
    got, dbg = _one(day, elevated(11.5))
    assert dbg[0] == BRANCH_EDGE and (got < np.array([3.0, 2.5, 1.5], F)).all() and (got > _f64_sky(s_day, np.sin(np.radians(11.5)), 0.9996)).all()
    assert _one(day, elevated(13.0))[1][0] == BRANCH_NONE


def test_cubemap_known_answers():
    lut = P._powf_table()
    odd = make_faces(9, ODD_SIZES)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    for intensity in (1.0, 0.37):
        sky = cubemap_sky(odd, intensity)
        for f, d in enumerate(axes):
            # a face's centre: u = v = 0.5 falls on the centre texel of an odd-sized face with both weights 0
            got, dbg = _one(sky, tuple(5.0 * v for v in d))
            h, w = odd[f].rgba.shape[:2]
            want = lut[odd[f].rgba[(h - 1) // 2, (w - 1) // 2, :3]] * F(intensity)
            assert np.array_equal(got, want.astype(F)) and dbg == (f, 0), (f, got, want)
    sky = cubemap_sky()
    faces = make_faces()
    # the 1 x 1 face (+Y) returns its texel from every direction that chooses it
    for d in ((0, 1, 0), (0.3, 1, -0.9), (-0.5, 1, 1), (0.999, 1, 0)):
        got, dbg = _one(sky, d)
        assert np.array_equal(got, lut[faces[2].rgba[0, 0, :3]]) and dbg[0] == 2, d
    # ties: ax >= ay && ax >= az is asked first, then ay >= ax && ay >= az
    for d, face in (((1, 1, 0), 0), ((-1, 1, 0), 1), ((0, 1, -1), 2), ((0, -1, 1), 3), ((-1, 0, 1), 1), ((2, 2, 2), 0), ((-2, -2, -2), 1),
                    ((1, -1, 1), 0), ((-1, -1, 1), 1), ((0, 0.5, 0.5), 2)):
        assert _one(sky, d)[1][0] == face, d
    # a face edge: (1, 1, 0) on +X has u = 0.5, v = 1, the last row, between the two middle columns of the 4 x 4 face
    got, _ = _one(sky, (1, 1, 0))
    a, b = lut[faces[0].rgba[3, 1, :3]], lut[faces[0].rgba[3, 2, :3]]
    assert np.array_equal(got, (a * F(0.5) + b * F(0.5)).astype(F))
    # the corner (1, 1, -1) on +X: u = v = 1, the last texel, nothing mixed in
    got, _ = _one(sky, (1, 1, -1))
    assert np.array_equal(got, lut[faces[0].rgba[3, 3, :3]])
    # a direction shorter than 1e-8 is black
    for d in ((0, 0, 0), (-0.0, 0.0, -0.0), (1e-9, -1e-9, 1e-9)):
        got, dbg = _one(sky, d)
        assert (got == 0).all() and dbg[0] == -1
    # a NaN or infinite direction weights the texels with NaN: every channel NaN, in bounds all the same
    got, _ = ref_samples(sky, nan_directions())
    assert np.isnan(got).all()


def test_background_goes_only_where_no_fragment_is_shown():
    """rsk_render_pbr is rcp_render plus the sky where tri_id < 0; composing in Python gives the same planes."""
    view, lvp, draws, mats = P.demo_scene()
    shadow = R.ref_shadow(R.SM, lvp, draws)
    frame = P.pbr_frame(view, lvp)
    plain = P.ref_render_pbr(frame, draws, mats, shadow, P.make_ibl())
    for _, sky in demo_skies():
        both = ref_render_pbr_sky(sky, frame, draws, mats, shadow, P.make_ibl())
        comp = ref_compose(sky, plain)
        covered = plain["tri_id"] >= 0
        for k in ("color", "depth", "velocity", "prequant", "tri_id"):
            assert np.array_equal(both[k].view(np.uint8), comp[k].view(np.uint8)), k
            assert np.array_equal(both[k][covered], plain[k][covered]), k
        alone = ref_compose(sky, None, W, H)
        assert np.array_equal(both["color"][~covered], alone["color"][~covered])
        assert np.array_equal(both["prequant"][~covered], alone["prequant"][~covered])
        assert (both["color"][~covered] != np.array(frame.clear_color, np.uint8)).any(-1).mean() > 0.99


# ---- what the GPU frames are there for -------------------------------------------------------------------

def test_frames_cover_what_the_gpu_tests_need():
    """On the restatement alone: the analytic frame shows the disc, the ring and the three bands of cosTheta; the cubemap
    frames sample all six faces; the demo's uncovered pixels include the disc and the ring under the analytic sky and
    more than one face under the cubemap."""
    skies = dict(frame_skies())
    dbg = ref_compose(skies["analytic-reinhard"], None, W, H)["sky_dbg"]
    n = {"disc": int((dbg[..., 0] == BRANCH_DISC).sum()), "ring": int((dbg[..., 0] == BRANCH_EDGE).sum()),
         "above": int((dbg[..., 1] == 2).sum()), "inside": int((dbg[..., 1] == 1).sum()), "below": int((dbg[..., 1] == 0).sum())}
    assert n["disc"] >= 8 and n["ring"] >= 20 and n["above"] >= 1000 and n["inside"] >= 1000 and n["below"] >= 1000, n
    down = ref_compose(skies["analytic-down"], None, W, H)["sky_dbg"]
    assert (down[..., 1] == 0).mean() > 0.6 and (down[..., 0] == BRANCH_NONE).all()
    faces = set()
    for name in ("cubemap-clamp", "cubemap-reinhard"):
        seen = np.bincount(ref_compose(skies[name], None, W, H)["sky_dbg"][..., 0].ravel(), minlength=6)
        assert (seen > 0).sum() >= 3, (name, seen)
        faces |= set(np.flatnonzero(seen >= 50).tolist())
    assert faces == set(range(6))
    view, lvp, draws, mats = P.demo_scene()
    plain = P.ref_render_pbr(P.pbr_frame(view, lvp), draws, mats, R.ref_shadow(R.SM, lvp, draws), P.make_ibl())
    open_px = plain["tri_id"] < 0
    assert 3000 < open_px.sum() < W * H - 3000
    demo = dict(demo_skies())
    a = ref_compose(demo["analytic"], plain)["sky_dbg"][open_px]
    assert (a[:, 0] == BRANCH_DISC).sum() >= 4 and (a[:, 0] == BRANCH_EDGE).sum() >= 10 and len(set(a[:, 1].tolist())) >= 2
    c = ref_compose(demo["cubemap"], plain)["sky_dbg"][open_px]
    assert len(set(c[:, 0].tolist())) >= 2
