"""The scene's sky model behind the meshes (pass_pbr_forward.hpp:64-73): ProceduralSky, CubemapSky and
render_skybox_to_hdr on the GPU (shs_lib_set_sky, shs_sky_sample) against the line-cited C restatement
tests/sky_ref/ref_sky.c -- bit for bit: the sun disc edge, the face choice and the texel floor are
discontinuities that a tolerance would hide.

CPU: the restatement pinned by an independent float32 numpy version (directions vectorised, GLM's operation
orders written out, the sRGB table from the host's powf) and hand-computed known answers.  GPU: sampled
directions and rendered frames equal the restatement; covered pixels, depth and motion equal the same frame
without a sky; small frames, both tonemaps, the light shafts after it, sharded frames, a re-issued pass and
the group call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "sky_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_sky_ref.so")
F = np.float32
_P = ctypes.c_void_p
_ref = None
PROCEDURAL, CUBEMAP = 1, 2


class RefSkyC(ctypes.Structure):
    _fields_ = [("model", ctypes.c_int32), ("sun_dir_ws", ctypes.c_float * 3), ("intensity", ctypes.c_float),
                ("fw", ctypes.c_int32 * 6), ("fh", ctypes.c_int32 * 6), ("face", ctypes.c_void_p * 6)]


def ref_lib():
    """libshs_sky_ref.so, built by make as tests/test_light_shafts.py builds its own."""
    global _ref
    if _ref is None:
        subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
        L = ctypes.CDLL(REF_LIB)
        L.ref_inverse.restype = None
        L.ref_inverse.argtypes = [_P, _P]
        L.ref_sky_sample.restype = None
        L.ref_sky_sample.argtypes = [ctypes.POINTER(RefSkyC), _P, ctypes.c_int, _P]
        L.ref_sky_fill.restype = None
        L.ref_sky_fill.argtypes = [ctypes.POINTER(RefSkyC), _P, _P, ctypes.c_int, ctypes.c_int, _P]
        _ref = L
    return _ref


def _ref_desc(sky):
    """lib_path.LibSky -> (RefSkyC, the arrays it points into)."""
    d = RefSkyC()
    d.model = int(sky.model)
    d.sun_dir_ws[:] = [float(F(v)) for v in sky.sun_dir_ws]
    d.intensity = float(F(sky.intensity))
    keep = []
    if sky.model == CUBEMAP and sky.faces is not None:
        for k, t in enumerate(sky.faces):
            if t is None:
                continue
            a = np.ascontiguousarray(t.rgba, dtype=np.uint8)
            keep.append(a)
            d.face[k], d.fw[k], d.fh[k] = a.ctypes.data, a.shape[1], a.shape[0]
    return d, keep


def ref_sample(sky, dirs):
    dirs = np.ascontiguousarray(np.asarray(dirs, F).reshape(-1, 3))
    out = np.zeros_like(dirs)
    d, _keep = _ref_desc(sky)
    ref_lib().ref_sky_sample(ctypes.byref(d), dirs.ctypes.data, dirs.shape[0], out.ctypes.data)
    return out


def ref_fill(sky, W, H):
    out = np.full((H, W, 4), -7.0, F)
    d, _keep = _ref_desc(sky)
    vp = np.ascontiguousarray(np.asarray(sky.cam_viewproj, F).reshape(16))
    cam = np.ascontiguousarray(np.asarray(sky.cam_pos, F).reshape(3))
    ref_lib().ref_sky_fill(ctypes.byref(d), vp.ctypes.data, cam.ctypes.data, W, H, out.ctypes.data)
    return out


def same_bits(a, b):
    """Bit-equal, a NaN matching any NaN (ProceduralSky of a zero direction)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- float32 numpy restatement of the cited lines (independent of the C text) -----------------------
def _gmin(x, y):
    return np.where(y < x, y, x)            # glm::min


def _gmax(x, y):
    return np.where(x < y, y, x)            # glm::max


def _gclamp(x, lo, hi):
    return _gmin(_gmax(x, F(lo)), F(hi))


def _mix(x, y, a):
    return x * (F(1.0) - a) + y * a


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    return v * (F(1.0) / np.sqrt(_dot(v, v)))[..., None]


_lut = None


def srgb_lut():
    """std::pow((float)c / 255.0f, 2.2f) for c = 0..255 from the host's libm: the table the library uploads."""
    global _lut
    if _lut is None:
        m = ctypes.CDLL("libm.so.6")
        m.powf.restype = ctypes.c_float
        m.powf.argtypes = [ctypes.c_float, ctypes.c_float]
        _lut = np.array([m.powf(float(F(c) / F(255.0)), float(F(2.2))) for c in range(256)], F)
        exact = (np.arange(256, dtype=np.float64) / 255.0).astype(F).astype(np.float64) ** float(F(2.2))
        assert np.all(np.abs(_lut.astype(np.float64) - exact) <= np.spacing(exact.astype(F)))
    return _lut


def np_procedural(sun_dir_ws, dirs):
    with np.errstate(all="ignore"):
        sun = _normalize(np.asarray(sun_dir_ws, F).reshape(3))
        d = _normalize(np.asarray(dirs, F).reshape(-1, 3))
        t = _gclamp(d[:, 1] * F(0.5) + F(0.5), 0.0, 1.0)
        zenith, horizon = np.array([0.05, 0.20, 0.50], F), np.array([0.30, 0.60, 1.00], F)
        sky = _mix(horizon[None, :], zenith[None, :], t[:, None])
        sun_dot = _dot(d, (-sun)[None, :])
        glow = (sun_dot - F(0.9990)) / (F(0.9998) - F(0.9990))
        ring = _mix(sky, np.array([10.0, 8.0, 4.0], F)[None, :], glow[:, None])
        out = np.where((sun_dot > F(0.9998))[:, None], F(15.0), np.where((sun_dot > F(0.9990))[:, None], ring, sky))
    assert out.dtype == F and sun_dot.dtype == F
    return out, sun_dot


def np_cube_face_uv(dirs):
    """-> (face or -1 for the zero vector, u, v in [0, 1] before the sampler's clamp)."""
    d = np.asarray(dirs, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ln = np.sqrt(_dot(d, d))
        zero = ln < F(1e-8)
        d = d / ln[:, None]
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        cx = (ax >= ay) & (ax >= az)
        cy = ~cx & (ay >= ax) & (ay >= az)
        face = np.where(cx, np.where(x > 0, 0, 1), np.where(cy, np.where(y > 0, 2, 3), np.where(z > 0, 4, 5)))
        us = [-z / ax, z / ax, x / ay, x / ay, x / az, -x / az]
        vs = [y / ax, y / ax, -z / ay, z / ay, y / az, y / az]
        u = np.choose(face, us)
        v = np.choose(face, vs)
        u = F(0.5) * (u + F(1.0))
        v = F(0.5) * (v + F(1.0))
    return np.where(zero, -1, face), u.astype(F), v.astype(F)


def np_cubemap(faces, intensity, dirs):
    lut = srgb_lut()
    face, u, v = np_cube_face_uv(dirs)
    out = np.zeros((face.size, 3), F)
    if any(t is None for t in faces):
        return out                                        # an invalid cubemap
    for k in range(6):
        sel = face == k
        if not sel.any():
            continue
        tex = np.asarray(faces[k].rgba, np.uint8)
        h, w = tex.shape[:2]
        uu, vv = _gclamp(u[sel], 0.0, 1.0), _gclamp(v[sel], 0.0, 1.0)
        fx, fy = uu * F(w - 1), vv * F(h - 1)
        x0, y0 = np.floor(fx).astype(np.int32), np.floor(fy).astype(np.int32)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        tx, ty = (fx - x0.astype(F))[:, None], (fy - y0.astype(F))[:, None]
        v00, v10, v01, v11 = (lut[tex[yy, xx, :3]] for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
        out[sel] = _mix(_mix(v00, v10, tx), _mix(v01, v11, tx), ty) * F(intensity)
    assert out.dtype == F
    return out


def np_sample(sky, dirs):
    if sky.model == PROCEDURAL:
        return np_procedural(sky.sun_dir_ws, dirs)[0]
    return np_cubemap(sky.faces, sky.intensity, dirs)


def np_inverse(m):
    """glm::inverse(mat4) (func_matrix.inl compute_inverse<4, 4>), column-major, float32 scalars."""
    m = [F(v) for v in np.asarray(m, F).reshape(16)]

    def M(c, r):
        return m[c * 4 + r]

    def sub(a, b, c, d):   # M a * M b - M c * M d
        return F(F(M(*a) * M(*b)) - F(M(*c) * M(*d)))
    with np.errstate(all="ignore"):
        c00 = sub((2, 2), (3, 3), (3, 2), (2, 3)); c02 = sub((1, 2), (3, 3), (3, 2), (1, 3)); c03 = sub((1, 2), (2, 3), (2, 2), (1, 3))
        c04 = sub((2, 1), (3, 3), (3, 1), (2, 3)); c06 = sub((1, 1), (3, 3), (3, 1), (1, 3)); c07 = sub((1, 1), (2, 3), (2, 1), (1, 3))
        c08 = sub((2, 1), (3, 2), (3, 1), (2, 2)); c10 = sub((1, 1), (3, 2), (3, 1), (1, 2)); c11 = sub((1, 1), (2, 2), (2, 1), (1, 2))
        c12 = sub((2, 0), (3, 3), (3, 0), (2, 3)); c14 = sub((1, 0), (3, 3), (3, 0), (1, 3)); c15 = sub((1, 0), (2, 3), (2, 0), (1, 3))
        c16 = sub((2, 0), (3, 2), (3, 0), (2, 2)); c18 = sub((1, 0), (3, 2), (3, 0), (1, 2)); c19 = sub((1, 0), (2, 2), (2, 0), (1, 2))
        c20 = sub((2, 0), (3, 1), (3, 0), (2, 1)); c22 = sub((1, 0), (3, 1), (3, 0), (1, 1)); c23 = sub((1, 0), (2, 1), (2, 0), (1, 1))
        f = [np.array(v, F) for v in ((c00, c00, c02, c03), (c04, c04, c06, c07), (c08, c08, c10, c11),
                                      (c12, c12, c14, c15), (c16, c16, c18, c19), (c20, c20, c22, c23))]
        v = [np.array([M(1, r), M(0, r), M(0, r), M(0, r)], F) for r in range(4)]
        sa, sb = np.array([1, -1, 1, -1], F), np.array([-1, 1, -1, 1], F)
        inv = [((v[1] * f[0] - v[2] * f[1]) + v[3] * f[2]) * sa, ((v[0] * f[0] - v[2] * f[3]) + v[3] * f[4]) * sb,
               ((v[0] * f[1] - v[1] * f[3]) + v[3] * f[5]) * sa, ((v[0] * f[2] - v[1] * f[4]) + v[2] * f[5]) * sb]
        d = [F(M(0, r) * inv[r][0]) for r in range(4)]
        one_over = F(1.0) / F(F(d[0] + d[1]) + F(d[2] + d[3]))
        out = np.concatenate([col * one_over for col in inv]).astype(F)
    return out


def np_fill(sky, W, H):
    inv = np_inverse(sky.cam_viewproj)
    cam = np.asarray(sky.cam_pos, F).reshape(3)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        nx = (F(2.0) * (xs.astype(F) + F(0.5)) / F(W)) - F(1.0)
        ny = (F(2.0) * (ys.astype(F) + F(0.5)) / F(H)) - F(1.0)
        world = [(inv[r] * nx + inv[4 + r] * ny) + (inv[8 + r] * F(1.0) + inv[12 + r] * F(1.0)) for r in range(4)]
        small = np.abs(world[3]) < F(1e-8)
        p = np.stack([world[k] / world[3] - cam[k] for k in range(3)], axis=-1).astype(F)
        dirs = _normalize(p).reshape(-1, 3)
        rgb = np_sample(sky, dirs).reshape(H, W, 3)
    out = np.ones((H, W, 4), F)
    out[..., :3] = np.where(small[..., None], F(0.0), rgb)
    return out, dirs.reshape(H, W, 3), small


# ---- direction sets and skies -----------------------------------------------------------------------
def _tex(rng, w, h):
    from shs_gpu.lib_path import Texture2D
    return Texture2D(rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8))


FACE_SETS = {"1x1": [(1, 1)] * 6, "2x2": [(2, 2)] * 6, "3x5": [(3, 5)] * 6,
             "mixed": [(1, 1), (2, 2), (3, 5), (4, 4), (5, 3), (8, 2)]}
_skies = {}


def cube_sky(name, intensity=1.75):
    from shs_gpu.lib_path import LibSky
    if name not in _skies:
        rng = np.random.default_rng(sum(map(ord, name)))
        _skies[name] = [_tex(rng, w, h) for w, h in FACE_SETS[name]]
    return LibSky(model=CUBEMAP, faces=_skies[name], intensity=intensity)


SUN = (0.4668, -0.3487, 0.8127)


def proc_sky(sun=SUN):
    from shs_gpu.lib_path import LibSky
    return LibSky(model=PROCEDURAL, sun_dir_ws=tuple(float(v) for v in sun))


def _ulp_step(v, k):
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf if k > 0 else -np.inf), dtype=F)
    return v


def threshold_dirs(sun=SUN):
    """Directions whose sun_dot sweeps 0.9990f and 0.9998f: cos(angle) in steps of 1e-8 (under the 6e-8 ulp) in
    float64, then the one nearest each threshold with each component stepped by single ulps."""
    s = -np.asarray(sun, np.float64) / np.linalg.norm(sun)
    perp = np.cross(s, [0.0, 1.0, 0.0])
    perp /= np.linalg.norm(perp)
    out = []
    for thr in (0.9990, 0.9998):
        c = float(F(thr)) + np.arange(-300, 301) * 1e-8
        sweep = (c[:, None] * s[None, :] + np.sqrt(1.0 - c * c)[:, None] * perp[None, :]).astype(F) * F(3.0)
        out.append(sweep)
        base = sweep[300]
        for axis in range(3):
            for k in range(-40, 41):
                d = base.copy()
                d[axis] = _ulp_step(d[axis], k)
                out.append(d[None, :])
    return np.concatenate(out).astype(F)


def tie_dirs():
    """ax == ay, ay == az, ax == az, all equal, with every sign: the >= face choice, u / v exactly 0 and 1."""
    out = []
    for a, b, c in ((1.0, 1.0, 0.5), (0.5, 1.0, 1.0), (1.0, 0.5, 1.0), (1.0, 1.0, 1.0), (0.25, 0.25, 0.25), (3.0, 3.0, 1.0)):
        for sx in (1, -1):
            for sy in (1, -1):
                for sz in (1, -1):
                    out.append((sx * a, sy * b, sz * c))
    out += [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0, 0), (1e-9, 0, 0), (0, -2e-9, 1e-9)]
    return np.array(out, F)


def direction_sets():
    rng = np.random.default_rng(0x5C1)
    rnd = np.concatenate([rng.normal(size=(1200, 3)), rng.normal(size=(300, 3)) * 1e-3, rng.normal(size=(300, 3)) * 1e4])
    return {"random": rnd.astype(F), "thresholds": threshold_dirs(), "ties": tie_dirs()}


def all_skies():
    return [("procedural", proc_sky())] + [("cube_" + n, cube_sky(n)) for n in FACE_SETS]


# ---- CPU 1: the restatement pinned by the numpy version ---------------------------------------------
def test_inverse_restatement_equals_numpy_version():
    from shs_gpu.lib_path import look_at_lh, mat_mul, perspective_lh_no
    rng = np.random.default_rng(7)
    mats = [rng.normal(size=16).astype(F) for _ in range(50)]
    mats.append(mat_mul(perspective_lh_no(F(1.0), F(1.76), 0.1, 200.0), look_at_lh((0.0, 7.0, -16.0), (0.0, 1.5, 0.0))))
    mats.append(np.diag([1, 1, 1, 1e9]).astype(F).reshape(16))
    for m in mats:
        got = np.zeros(16, F)
        m = np.ascontiguousarray(m, F)
        ref_lib().ref_inverse(m.ctypes.data, got.ctypes.data)
        assert same_bits(got, np_inverse(m)), m


@pytest.mark.parametrize("which", ["random", "thresholds", "ties"])
def test_sampler_restatement_equals_numpy_version(which):
    dirs = direction_sets()[which]
    for name, sky in all_skies():
        got, want = ref_sample(sky, dirs), np_sample(sky, dirs)
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
        assert bad.size == 0, (name, which, dirs[bad[:3]], got[bad[:3]], want[bad[:3]])


def test_direction_sets_reach_the_discontinuities():
    sets = direction_sets()
    _, sd = np_procedural(SUN, sets["thresholds"])
    for thr in (F(0.9990), F(0.9998)):   # both sides of each threshold within 2 ulps, and the value itself
        near = sd[np.abs(sd - thr) <= 2 * np.spacing(thr)]
        assert (near > thr).any() and (near < thr).any() and (near == thr).any(), thr
    rgb, _ = np_procedural(SUN, sets["thresholds"])
    assert (rgb[:, 0] == 15).any() and ((rgb[:, 0] > 1.0) & (rgb[:, 0] < 15)).any() and (rgb[:, 0] < 1.0).any()
    assert np.isnan(np_procedural(SUN, np.zeros((1, 3), F))[0]).all()          # normalize(0): the legitimate NaN
    face, u, v = np_cube_face_uv(sets["ties"])
    assert set(face.tolist()) == {-1, 0, 1, 2, 3, 4, 5} and (face == -1).sum() == 3
    assert ((u == 0) & (face >= 0)).any() and ((u == 1) & (face >= 0)).any()
    assert ((v == 0) & (face >= 0)).any() and ((v == 1) & (face >= 0)).any()
    face_r, _, _ = np_cube_face_uv(sets["random"])
    assert np.bincount(face_r, minlength=6).min() > 100
    # written order of the ties: ax == ay >= az takes X, ay == az > ax takes Y
    assert np_cube_face_uv(np.array([[1, 1, 0.5], [-1, 1, 1], [0.5, 1, 1], [0.5, -1, 1]], F))[0].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("size", [(97, 61), (17, 9), (37, 1), (1, 29), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fill_restatement_equals_numpy_version(size):
    W, H = size
    for name, sky in all_skies():
        _camera_scene(W, H, sky)
        want, _, small = np_fill(sky, W, H)
        assert not small.any()
        assert same_bits(ref_fill(sky, W, H), want), (name, size)


# ---- CPU 2: hand-computed known answers ----------------------------------------------------------------
def test_known_answers():
    from shs_gpu.lib_path import LibSky, Texture2D
    sky = proc_sky()
    up_down = ref_sample(sky, [(0, 1, 0), (0, -5, 0)])
    assert same_bits(up_down[0], [0.05, 0.20, 0.50]) and same_bits(up_down[1], [0.30, 0.60, 1.00])   # zenith, horizon
    s = np.asarray(SUN, np.float64)
    assert same_bits(ref_sample(sky, [tuple(-s), tuple(-7 * s)]), np.full((2, 3), 15.0, F))             # at the sun
    assert ref_sample(sky, [tuple(s)])[0, 0] < 1.0                                                      # away from it
    texel = np.array([[[255, 128, 0, 9]]], np.uint8)
    one = LibSky(model=CUBEMAP, faces=[Texture2D(texel)] * 6, intensity=2.0)
    lut = srgb_lut()
    want = np.array([lut[255], lut[128], lut[0]], F) * F(2.0)
    assert lut[255] == 1.0 and lut[0] == 0.0 and abs(float(lut[128]) - (128 / 255) ** 2.2) < 1e-7
    for d in direction_sets()["random"][:50]:
        assert same_bits(ref_sample(one, [d])[0], want)
    assert not ref_sample(one, [(0, 0, 0)]).any()                      # len < 1e-8
    broken = LibSky(model=CUBEMAP, faces=[Texture2D(texel)] * 5 + [None], intensity=2.0)
    assert not ref_sample(broken, direction_sets()["random"][:50]).any() and not np_cubemap(broken.faces, 2.0, [(1, 2, 3)]).any()
    # world.w = 1e-9 for every pixel: the |w| < 1e-8 guard
    for model_sky in (proc_sky(), one):
        model_sky.cam_viewproj = np.diag([1, 1, 1, 1e9]).astype(F).reshape(16)
        got = ref_fill(model_sky, 13, 7)
        assert same_bits(got, np.broadcast_to(np.array([0, 0, 0, 1], F), (7, 13, 4)))
        assert same_bits(np_fill(model_sky, 13, 7)[0], got)
    # identity camera at the origin, a 2x2 frame: dir = normalize(ndc, 1) with ndc = +-0.5
    ident = proc_sky()
    got = ref_fill(ident, 2, 2)
    dirs = np.array([[[-0.5, -0.5, 1], [0.5, -0.5, 1]], [[-0.5, 0.5, 1], [0.5, 0.5, 1]]], F)
    assert same_bits(got[..., :3], ref_sample(ident, _normalize(dirs.reshape(-1, 3))).reshape(2, 2, 3)) and (got[..., 3] == 1).all()
    assert got[1, 0, 2] < got[0, 0, 2]                                  # row 1 looks up: nearer the zenith's blue 0.5


# ---- CPU 3: the ABI surface ----------------------------------------------------------------------------
def test_abi_surface():
    import shs_gpu
    from shs_gpu import _abi
    L = shs_gpu.lib()
    for name in ("shs_lib_set_sky", "shs_sky_sample", "shs_group_lib_set_sky"):
        assert getattr(L, name).restype is ctypes.c_int
    assert L.shs_abi_version() == 1
    assert ctypes.sizeof(_abi.SkyDescC) == 4 * (1 + 16 + 3 + 3 + 6 + 1)
    header = open(os.path.join(os.path.dirname(HERE), "include", "shs_gpu.h")).read()
    for name, val in (("SHS_SKY_NONE", 0), ("SHS_SKY_PROCEDURAL", 1), ("SHS_SKY_CUBEMAP", 2)):
        assert f"#define {name} {val}\n" in header
    assert (_abi.SKY_NONE, _abi.SKY_PROCEDURAL, _abi.SKY_CUBEMAP) == (0, 1, 2)
    assert callable(shs_gpu.Context.set_sky) and callable(shs_gpu.Context.sky_sample)
    from shs_gpu.group import Group
    assert callable(Group.set_sky)
    # without a context nothing is set or sampled
    d = proc_sky().desc()
    assert L.shs_lib_set_sky(None, ctypes.byref(d)) == _abi.SHS_ERR_INVALID
    assert L.shs_sky_sample(None, ctypes.byref(d), None, 0, None) == _abi.SHS_ERR_INVALID
    assert L.shs_group_lib_set_sky(None, ctypes.byref(d)) == _abi.SHS_ERR_INVALID


# ---- the scene ---------------------------------------------------------------------------------------
EYE, LOOK_AT = (-10.0, 0.5, -10.0), (0.0, 6.0, 0.0)
SUN_AT = (1.0, 11.5, 4.0)           # a point the sun lies behind: in the sky above Suzanne


def _aim(eye, P):
    """sun_dir = -normalize(P - eye), as tests/test_light_shafts.py::_aim."""
    d = np.asarray(P, np.float64) - np.asarray(eye, np.float64)
    return (-d / np.linalg.norm(d)).astype(F)


def _camera_scene(W, H, sky=None):
    """scene_lib.c5_scene seen from near the ground looking up past Suzanne: floor, mesh and sky in one frame,
    the cube corner (+X, +Y, +Z) on the screen.  Fills sky's camera fields."""
    from shs_gpu import scene_lib
    from shs_gpu.lib_path import look_at_lh, mat_mul, perspective_lh_no
    frame, draws = scene_lib.c5_scene(W, H)[:2]
    eye = tuple(F(v) for v in EYE)
    proj = perspective_lh_no(F(np.deg2rad(60.0)), F(W) / F(H), 0.1, 200.0)
    vp = mat_mul(proj, look_at_lh(eye, LOOK_AT))
    prev = mat_mul(proj, look_at_lh((F(-10.2), F(0.5), F(-9.8)), LOOK_AT))
    for d in draws:
        d.viewproj, d.prev_viewproj, d.camera_pos = vp, prev, eye
    if sky is not None:
        sky.cam_viewproj, sky.cam_pos = np.asarray(vp, F), eye
    return frame, draws, np.asarray(vp, F), np.asarray(eye, F)


def frame_skies():
    return [("procedural", proc_sky(_aim(EYE, SUN_AT))), ("cubemap", cube_sky("mixed"))]


# ---- GPU ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    try:
        yield c
    finally:
        c.set_sky(None)
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_sky_sample_exact(ctx, n):
    sets = direction_sets()
    dirs = np.concatenate([sets["ties"], sets["thresholds"][::7], sets["random"]])
    assert len(dirs) >= 1000
    for start in (0, len(sets["ties"]) - 3):           # n = 1: the first tie, then the zero vector
        d = dirs[start:start + n]
        for name, sky in all_skies():
            got, want = ctx.sky_sample(sky, d), ref_sample(sky, d)
            assert got.shape == (n, 3) and same_bits(got, want), (name, n, start)
    if n == 1000:                                       # every direction of every set, once
        for which, d in sets.items():
            for name, sky in all_skies():
                assert same_bits(ctx.sky_sample(sky, d), ref_sample(sky, d)), (name, which)


_plain = {}


def _plain_frame(ctx, W, H):
    """The scene without a sky (gradient background), once per size."""
    if (W, H) not in _plain:
        frame, draws, _, _ = _camera_scene(W, H)
        ctx.set_sky(None)
        ctx.render_pbr_forward(frame, draws)
        _plain[(W, H)] = ctx.resolve_lib()
    return _plain[(W, H)]


def _assert_sky_frame(got, plain, want_sky, what):
    hdr, depth, motion = got
    p_hdr, p_depth, p_motion = plain
    covered = p_depth < 1.0
    assert np.array_equal(depth.view(np.uint32), p_depth.view(np.uint32)), what
    assert np.array_equal(motion.view(np.uint32), p_motion.view(np.uint32)), what
    assert np.array_equal(hdr[covered].view(np.uint32), p_hdr[covered].view(np.uint32)), what
    bad = np.argwhere((hdr.view(np.uint32) != want_sky.view(np.uint32)).any(axis=2) & ~covered)
    assert bad.size == 0, f"{what}: {len(bad)} sky pixels differ, first {bad[:4]}"
    return covered


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(352, 200), (97, 61)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rendered_frames_exact(ctx, size):
    W, H = size
    plain = _plain_frame(ctx, W, H)
    for name, sky in frame_skies():
        frame, draws, _, _ = _camera_scene(W, H, sky)
        want = ref_fill(sky, W, H)
        ctx.set_sky(sky)
        ctx.render_pbr_forward(frame, draws)
        covered = _assert_sky_frame(ctx.resolve_lib(), plain, want, (name, size))
        # the plain frame's background is the gradient: the sky frame ignored it
        assert not np.array_equal(plain[0][~covered], want[~covered])
        # non-vacuous, on the restatement's own output
        blocks = covered[:H - H % 4, :W - W % 16].reshape(H // 4, 4, W // 16, 16).sum(axis=(1, 3))
        assert (blocks == 0).any() and ((blocks > 0) & (blocks < 64)).any() and (blocks == 64).any(), (name, size)
        if size == (352, 200) and name == "procedural":
            disc = (want[..., 0] == 15) & ~covered
            glow = (want[..., 0] > 1.0) & (want[..., 0] < 15) & ~covered
            assert disc.sum() >= 20 and glow.sum() >= 20, (int(disc.sum()), int(glow.sum()))
        if name == "cubemap":
            _, dirs, _ = np_fill(sky, W, H)
            faces = np_cube_face_uv(dirs.reshape(-1, 3))[0].reshape(H, W)[~covered]
            assert len(set(faces.tolist())) >= 3, set(faces.tolist())
    ctx.set_sky(None)


@pytest.mark.gpu
def test_small_frames_in_one_context():
    """Sky, gradient, SHS_SKY_NONE by a descriptor and clear_hdr in turn: a stale sky would show."""
    import shs_gpu
    from shs_gpu.lib_path import LibSky
    with shs_gpu.Context(0) as c:
        k = 0
        for W, H in [(1, 1), (37, 1), (1, 29), (17, 9)]:
            frame, draws, _, _ = _camera_scene(W, H)
            c.set_sky(None)
            c.render_pbr_forward(frame, draws)
            plain = c.resolve_lib()
            covered = plain[1] < 1.0
            for name, sky in frame_skies():
                _camera_scene(W, H, sky)
                c.set_sky(sky)
                c.render_pbr_forward(frame, draws)
                _assert_sky_frame(c.resolve_lib(), plain, ref_fill(sky, W, H), (name, W, H))
                c.set_sky(None if k % 2 == 0 else LibSky(model=0))
                k += 1
                c.render_pbr_forward(frame, draws)
                for a, b in zip(c.resolve_lib(), plain):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, W, H)
                c.set_sky(sky)
                frame.bg_gradient, frame.clear_hdr = False, (0.25, 0.5, 0.75, 1.0)   # a sky frame ignores both
                c.render_pbr_forward(frame, draws)
                _assert_sky_frame(c.resolve_lib(), plain, ref_fill(sky, W, H), (name, W, H, "clear_hdr"))
                c.set_sky(None)
                c.render_pbr_forward(frame, draws)
                hdr = c.resolve_lib()[0]
                assert np.all(hdr[~covered] == np.array(frame.clear_hdr, F)), (name, W, H)
                frame.bg_gradient = True


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
def test_tonemap_sees_the_sky(ctx, oracle_mod, fused):
    W, H = 97, 61
    uncovered = ~(_plain_frame(ctx, W, H)[1] < 1.0)
    try:
        for name, sky in frame_skies():
            frame, draws, _, _ = _camera_scene(W, H, sky)
            ctx.set_sky(sky)
            ctx.fuse_tonemap(1.3, 2.2, ldr=True, present=True, enable=fused)
            ctx.render_pbr_forward(frame, draws)
            if not fused:
                ctx.tonemap(1.3, 2.2, ldr=True, present=True)
            ldr, pre = ctx.resolve_ldr()
            hdr = ctx.resolve_lib()[0]
            assert uncovered.any() and same_bits(hdr[uncovered], ref_fill(sky, W, H)[uncovered])
            want_ldr, want_pre = oracle_mod.tonemap(hdr, 1.3, 2.2)
            assert np.array_equal(ldr, want_ldr) and np.array_equal(pre, want_pre), (name, fused)
    finally:
        ctx.fuse_tonemap(enable=False)
        ctx.set_sky(None)


@pytest.mark.gpu
def test_light_shafts_find_the_sun(ctx, oracle_mod):
    """Sky -> tonemap -> light_shafts: the pass marches towards a sun that is now in the frame."""
    from test_light_shafts import ref_shafts
    W, H = 352, 200
    sky = proc_sky(_aim(EYE, SUN_AT))
    frame, draws, vp, eye = _camera_scene(W, H, sky)
    sun = np.asarray(sky.sun_dir_ws, F)
    uv, valid = ctx.light_shafts_sun_uv(vp, eye, sun)
    assert valid
    plain_hdr = _plain_frame(ctx, W, H)[0]
    try:
        ctx.set_sky(sky)
        ctx.render_pbr_forward(frame, draws)
        ctx.tonemap(1.0, 2.2)
        base, _ = ctx.resolve_ldr()
        hdr, depth, _ = ctx.resolve_lib()
        assert np.array_equal(base, oracle_mod.tonemap(hdr, 1.0, 2.2)[0])
        ctx.light_shafts(vp, eye, sun, weight=0.05)
        got, pre = ctx.resolve_ldr()
    finally:
        ctx.set_sky(None)
    want, boost, ran = ref_shafts(base, depth, vp, eye, sun, weight=0.05)
    assert ran and np.array_equal(got, want) and np.array_equal(pre, got[::-1])
    sx, sy = int(round(float(uv[0]) * (W - 1))), int(round(float(uv[1]) * (H - 1)))
    assert ref_fill(sky, W, H)[sy, sx, 0] == 15                     # the disc is where the pass looks
    assert boost[max(sy - 6, 0):sy + 7, max(sx - 6, 0):sx + 7].min() > 0
    # the same chain over the gradient has less to add there
    _, plain_boost, _ = ref_shafts(oracle_mod.tonemap(plain_hdr, 1.0, 2.2)[0], depth, vp, eye, sun, weight=0.05)
    assert boost[sy, sx] > plain_boost[sy, sx]


def _tile_owner(W, H, count):
    ys, xs = np.mgrid[0:H, 0:W]
    return ((ys // 32) * ((W + 31) // 32) + xs // 32) % count


@pytest.mark.gpu
def test_tile_sharded_frames(ctx):
    W, H, count = 352, 200, 3
    owner = _tile_owner(W, H, count)
    plain = _plain_frame(ctx, W, H)
    try:
        for name, sky in frame_skies():
            frame, draws, _, _ = _camera_scene(W, H, sky)
            ctx.set_sky(sky)
            ctx.render_pbr_forward(frame, draws)
            whole = ctx.resolve_lib()
            _assert_sky_frame(whole, plain, ref_fill(sky, W, H), name)
            for r in range(count):
                frame.shard_rank, frame.shard_count = r, count
                ctx.render_pbr_forward(frame, draws)
                own = owner == r
                for a, b in zip(ctx.resolve_lib(), whole):
                    assert np.array_equal(a[own].view(np.uint32), b[own].view(np.uint32)), (name, r)
    finally:
        ctx.set_sky(None)


@pytest.mark.gpu
def test_region_sharded_frames():
    """The region layout set up as tests/test_regions.py does: one context per rank, SHS_SHARD_REGIONS, two
    frames (the second split from the first's block bounds)."""
    import shs_gpu
    W, H, count = 352, 200, 3
    name, sky = frame_skies()[0]
    frame, draws, _, _ = _camera_scene(W, H, sky)
    want = ref_fill(sky, W, H)
    ctxs = [shs_gpu.Context(0) for _ in range(count)]
    try:
        ctxs[0].set_sky(sky)
        ctxs[0].render_pbr_forward(frame, draws)
        whole = ctxs[0].resolve_lib()
        for c in ctxs:
            c.set_shard_layout(True)
            c.set_sky(sky)
        for it in range(2):
            seen = np.zeros((H, W), np.int32)
            for r, c in enumerate(ctxs):
                frame.shard_rank, frame.shard_count = r, count
                c.render_pbr_forward(frame, draws)
                got = c.resolve_lib()
                x0, y0, x1, y1 = c.shard_regions(count)[r]
                own = np.zeros((H, W), bool)
                if x1 >= x0 and y1 >= y0:
                    own[y0 * 32:(y1 + 1) * 32, x0 * 32:(x1 + 1) * 32] = True
                seen += own
                for a, b in zip(got, whole):
                    assert np.array_equal(a[own].view(np.uint32), b[own].view(np.uint32)), (it, r)
                unc = own & ~(whole[1] < 1.0)
                assert same_bits(got[0][unc], want[unc])
            assert (seen == 1).all()
    finally:
        frame.shard_rank, frame.shard_count = 0, 1
        for c in ctxs:
            c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["procedural", "cubemap"])
def test_reissued_camera_pass_replays_its_sky(model):
    """The overflow re-issue scene of tests/test_light_shafts.py: the first camera pass of a fresh context
    overflows the spill capacity.  Another sky is set before anything is resolved: the re-issue paints the sky
    the pass was enqueued with."""
    import shs_gpu
    from shs_gpu.lib_path import look_at_lh, mat_mul, perspective_lh_no
    from test_light_shafts import RH, RW, _ten_stacks
    frame, draws = _ten_stacks()
    sky = dict(frame_skies())[model]
    other = proc_sky((0.0, -1.0, 0.0))
    eye = (F(0.0), F(1.0), F(-5.0))
    for s in (sky, other):
        s.cam_viewproj = np.asarray(mat_mul(perspective_lh_no(F(1.0), F(RW) / F(RH), 0.1, 200.0), look_at_lh(eye, (0.0, 2.0, 0.0))), F)
        s.cam_pos = eye
    if model == "procedural":
        sky.sun_dir_ws = tuple(float(v) for v in _aim(eye, (-1.0, 2.5, 0.0)))
    with shs_gpu.Context(0) as c:
        c.enable_timing(True)
        c.lib_timing_reset()
        c.set_sky(sky)
        c.render_pbr_forward(frame, draws)
        c.set_sky(other)
        hdr, depth, _ = c.resolve_lib()
        n_pass, _ = c.lib_timing_read()
        assert n_pass["camera"] == 2, n_pass
        c.set_sky(None)
        c.render_pbr_forward(frame, draws)
        plain = c.resolve_lib()
    covered = plain[1] < 1.0
    want = ref_fill(sky, RW, RH)
    assert covered.any() and (~covered).sum() > 1000
    assert not same_bits(want[~covered], ref_fill(other, RW, RH)[~covered])
    assert np.array_equal(depth.view(np.uint32), plain[1].view(np.uint32))
    assert np.array_equal(hdr[covered].view(np.uint32), plain[0][covered].view(np.uint32))
    assert same_bits(hdr[~covered], want[~covered])
    if model == "procedural":
        assert (want[~covered][:, 0] == 15).sum() >= 20


@pytest.mark.gpu
def test_group_set_sky(ctx):
    from shs_gpu.group import Group
    W, H = 97, 61
    plain = _plain_frame(ctx, W, H)
    g = Group([0])
    try:
        for name, sky in frame_skies():
            frame, draws, _, _ = _camera_scene(W, H, sky)
            g.set_sky(sky)
            g.render_pbr_forward(frame, draws)
            g.gather(g.root.TARGET_LIB)
            _assert_sky_frame(g.root.resolve_lib(), plain, ref_fill(sky, W, H), name)
        g.set_sky(None)
        g.render_pbr_forward(frame, draws)
        g.gather(g.root.TARGET_LIB)
        for a, b in zip(g.root.resolve_lib(), plain):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        g.close()


@pytest.mark.gpu
def test_validation():
    import shs_gpu
    from shs_gpu import ShsError
    from shs_gpu.lib_path import LibSky, Texture2D
    with shs_gpu.Context(0) as c:
        good = proc_sky()
        c.set_sky(good)
        bad = [LibSky(model=3), LibSky(model=-1), proc_sky((0.0, 0.0, 0.0)), proc_sky((float("nan"), 1.0, 0.0)),
               LibSky(model=PROCEDURAL, cam_pos=(float("inf"), 0.0, 0.0)),
               LibSky(model=PROCEDURAL, cam_viewproj=np.zeros(16, F)),                      # singular: no finite inverse
               LibSky(model=PROCEDURAL, cam_viewproj=np.full(16, np.nan, F)),
               LibSky(model=CUBEMAP, faces=None),                                           # face ids 0
               LibSky(model=CUBEMAP, faces=cube_sky("2x2").faces, intensity=float("inf"))]
        for sky in bad:
            with pytest.raises(ShsError):
                c.set_sky(sky)
        d = cube_sky("2x2").desc([1, 2, 3, 4, 5, 99])                                       # an unknown id
        assert c._lib.shs_lib_set_sky(c._h, ctypes.byref(d)) != 0
        with pytest.raises(ShsError):
            c.sky_sample(LibSky(model=7), [(0, 1, 0)])
        # a face of the current sky cannot be released; after another sky is set it can
        cube = LibSky(model=CUBEMAP, faces=[Texture2D(np.full((2, 2, 4), 40 * k, np.uint8)) for k in range(6)])
        c.set_sky(cube)
        tid = c.upload_texture(cube.faces[3])
        assert c._lib.shs_texture_release(c._h, tid) != 0
        assert same_bits(c.sky_sample(cube, [(0, -1, 0)]), ref_sample(cube, [(0, -1, 0)]))
        c.set_sky(good)
        assert c._lib.shs_texture_release(c._h, tid) == 0
        d = cube.desc([c.upload_texture(t) if k != 3 else tid for k, t in enumerate(cube.faces)])
        assert c._lib.shs_lib_set_sky(c._h, ctypes.byref(d)) != 0                          # the released id
