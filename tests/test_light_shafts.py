"""PassLightShafts (pass_light_shafts.hpp:44-215) between tonemap and motion blur: shs_light_shafts
against the line-cited C restatement tests/light_shafts_ref/ref_light_shafts.c.

CPU: the host's sun projection, the restatement pinned by an independent float32 numpy version (steps
looped, pixels vectorised, lround through float64 with the (int)(long) wrap, clamps as comparisons) and
hand-computed known answers.  GPU: the LDR (and present staging) bytes equal the restatement's for
rendered and synthetic planes, degenerate sizes, the pass chain's order and a re-issued camera pass."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "light_shafts_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_light_shafts_ref.so")
F = np.float32
_P = ctypes.c_void_p
_ref = None


def ref_lib():
    """libshs_light_shafts_ref.so, built by make as tests/test_light_types_ref.py builds its own."""
    global _ref
    if _ref is None:
        subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
        L = ctypes.CDLL(REF_LIB)
        L.ref_sun_uv.restype = ctypes.c_int
        L.ref_sun_uv.argtypes = [_P] * 4
        fl = ctypes.c_float
        L.ref_light_shafts_uv.restype = ctypes.c_int
        L.ref_light_shafts_uv.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, fl, fl, fl, _P, _P]
        L.ref_light_shafts.restype = ctypes.c_int
        L.ref_light_shafts.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, fl, fl, fl, _P, _P, _P, _P]
        _ref = L
    return _ref


def _f32(a, n):
    return np.ascontiguousarray(np.asarray(a, F).reshape(n))


def ref_sun_uv(viewproj, cam_pos, sun_dir):
    uv = np.zeros(2, F)
    a = [_f32(cam_pos, 3), _f32(sun_dir, 3), _f32(viewproj, 16)]
    valid = ref_lib().ref_sun_uv(*[v.ctypes.data for v in a], uv.ctypes.data)
    return uv, bool(valid)


def _planes(ldr, depth):
    h, w = ldr.shape[:2]
    out = np.ascontiguousarray(ldr, dtype=np.uint8).copy()
    dp = None if depth is None else np.ascontiguousarray(depth, dtype=F)
    assert dp is None or dp.shape == (h, w)
    return out, dp, np.zeros((h, w), np.int32), w, h


def ref_shafts_uv(ldr, depth, sun_uv, steps=48, density=0.8, weight=0.9, decay=0.95):
    """The restatement's main loop with the sun given on the screen -> (ldr out, boost)."""
    out, dp, boost, w, h = _planes(ldr, depth)
    uv = _f32(sun_uv, 2)
    rc = ref_lib().ref_light_shafts_uv(out.ctypes.data, None if dp is None else dp.ctypes.data, w, h, int(steps), density,
                                       weight, decay, uv.ctypes.data, boost.ctypes.data)
    assert rc == 0
    return out, boost


def ref_shafts(ldr, depth, viewproj, cam_pos, sun_dir, enable=True, steps=48, density=0.8, weight=0.9, decay=0.95):
    """The whole pass as the adapter runs it (input == output) -> (ldr out, boost, whether the shafts ran)."""
    out, dp, boost, w, h = _planes(ldr, depth)
    a = [_f32(cam_pos, 3), _f32(sun_dir, 3), _f32(viewproj, 16)]
    rc = ref_lib().ref_light_shafts(out.ctypes.data, None if dp is None else dp.ctypes.data, w, h, 1 if enable else 0,
                                    int(steps), density, weight, decay, *[v.ctypes.data for v in a], boost.ctypes.data)
    assert rc in (0, 1)
    return out, boost, rc == 1


# ---- float32 numpy restatement of the cited lines (independent of the C text) -----------------------
def _lround_int(v):
    """(int)std::lround(float) on x86-64: half away from zero in 64 bits (NaN and |v| >= 2^63 give LONG_MIN),
    then the (int) cast keeps the low 32 bits."""
    v = np.asarray(v, F).astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = np.trunc(v + np.copysign(0.5, v))
        ok = np.abs(r) < 2.0 ** 63
    return np.where(ok, r, 0.0).astype(np.int64).astype(np.int32)


def _clamp(v, lo, hi):
    return np.where(v < lo, lo, np.where(hi < v, hi, v))   # std::clamp: a NaN passes through


def np_sun_uv(viewproj, cam_pos, sun_dir):
    m, c, d = _f32(viewproj, 16), _f32(cam_pos, 3), _f32(sun_dir, 3)
    with np.errstate(all="ignore"):
        p = [F(c[k] + F(F(-d[k]) * F(100.0))) for k in range(3)]
        clip = [F(F(F(m[r] * p[0]) + F(m[4 + r] * p[1])) + F(F(m[8 + r] * p[2]) + F(m[12 + r] * F(1.0)))) for r in range(4)]
        if not abs(clip[3]) > F(1e-6):
            return np.array([0.5, 0.2], F), False
        ndc = [F(clip[k] / clip[3]) for k in range(3)]
        uv = np.array([F(F(ndc[0] * F(0.5)) + F(0.5)), F(F(ndc[1] * F(0.5)) + F(0.5))], F)
    valid = bool(clip[3] > 0 and -1 <= ndc[2] <= 1 and 0 <= uv[0] <= 1 and 0 <= uv[1] <= 1)
    return uv, valid


def np_shafts_uv(ldr, depth, sun_uv, steps=48, density=0.8, weight=0.9, decay=0.95):
    h, w = ldr.shape[:2]
    rgb = ldr[..., :3].astype(F) / F(255.0)
    luma = (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]
    steps = max(8, int(steps))
    density, weight = max(F(0.0), F(density)), max(F(0.0), F(weight))
    decay = F(_clamp(F(decay), F(0.0), F(1.0)))
    ys, xs = np.mgrid[0:h, 0:w]
    u = xs.astype(F) / F(max(1, w - 1))
    v = ys.astype(F) / F(max(1, h - 1))
    su0, sv0 = F(sun_uv[0]), F(sun_uv[1])
    illum, accum = F(1.0), np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for i in range(steps):
            t = F(i) / F(steps)
            su = u + (su0 - u) * t * density
            sv = v + (sv0 - v) * t * density
            sx = _clamp(_lround_int(su * F(w - 1)), 0, w - 1)
            sy = _clamp(_lround_int(sv * F(h - 1)), 0, h - 1)
            s = luma[sy, sx]
            if depth is not None:
                s = s * _clamp(depth[sy, sx], F(0.0), F(1.0))
            accum = accum + s * illum * weight
            illum = F(illum * decay)
        boost = _clamp(_lround_int(accum * F(80.0)), 0, 120).astype(np.int32)
    assert accum.dtype == F and luma.dtype == F
    out = ldr.copy()
    b = ldr.astype(np.int32)
    out[..., 0] = np.minimum(b[..., 0] + boost, 255)
    out[..., 1] = np.minimum(b[..., 1] + boost, 255)
    out[..., 2] = np.minimum(b[..., 2] + boost // 2, 255)
    out[..., 3] = 255
    return out, boost


def _random_ldr(rng, w, h):
    return rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)


def _random_depth(rng, w, h, neg_inf=False):
    """[-0.2, 1.2] with 2 % NaN and 2 % +inf (and, for the device planes, 2 % -inf)."""
    d = rng.uniform(-0.2, 1.2, size=(h, w)).astype(F)
    r = rng.random((h, w))
    d[r < 0.02] = np.nan
    d[(r >= 0.02) & (r < 0.04)] = np.inf
    if neg_inf:
        d[(r >= 0.04) & (r < 0.06)] = -np.inf
    return d


# ---- CPU 1: the sun projection --------------------------------------------------------------------
def _c5_camera(W=352, H=200):
    from shs_gpu import scene_lib
    frame, draws, _casters, sun, _S = scene_lib.c5_scene(W, H)
    return frame, draws, np.asarray(draws[0].viewproj, F), np.asarray(draws[0].camera_pos, F), np.asarray(sun, F)


def _aim(eye, P):
    """sun_dir = -normalize(P - eye): the sun's far point lies on the ray from the eye through P."""
    d = np.asarray(P, np.float64) - np.asarray(eye, np.float64)
    return (-d / np.linalg.norm(d)).astype(F)


def _sun_cases():
    from shs_gpu.lib_path import look_at_lh, mat_mul, perspective_lh_no
    rng = np.random.default_rng(0x5AF7)
    ident = np.eye(4, dtype=F).reshape(16)
    cases = []
    for k in range(200):   # random cameras; a third of the suns aimed into the view, the rest anywhere
        eye = rng.uniform(-20, 20, 3).astype(F)
        at = (eye + rng.normal(size=3) * 10).astype(F)
        vp = mat_mul(perspective_lh_no(F(np.deg2rad(rng.uniform(30, 100))), F(rng.uniform(0.5, 2.5)), 0.1, F(rng.uniform(150, 500))),
                     look_at_lh(tuple(eye), tuple(at)))
        if k % 3 == 0:
            sun = _aim(eye, at + rng.normal(size=3) * 2)
        elif k % 3 == 1:
            sun = _aim(at, eye)                      # behind the camera
        else:
            sun = rng.normal(size=3).astype(F)
        cases.append((vp, eye, sun))
    zero_w = ident.copy()
    zero_w[[3, 7, 11, 15]] = 0                       # clip.w == 0
    cases.append((zero_w, np.zeros(3, F), np.array([0.0, 0.0, -0.005], F)))
    tiny_w = ident.copy()
    tiny_w[15] = 1e-6                                # |clip.w| == 1e-6f: not > 1e-6f
    cases.append((tiny_w, np.zeros(3, F), np.array([0.0, 0.0, 0.0], F)))
    # identity viewproj: clip = (sun_pos, 1).  ndc.z swept by single ulps of the direction across +1 and -1
    for sign in (1.0, -1.0):
        z0 = F(-0.01 * sign)
        for k in range(-60, 61):
            z = z0
            for _ in range(abs(k)):
                z = np.nextafter(z, F(np.sign(k) * sign * -1.0), dtype=F)
            cases.append((ident, np.zeros(3, F), np.array([0.0, 0.0, z], F)))
    # sun_uv exactly 1 and exactly 0 (cam_pos +-1, the direction adds +-0)
    cases.append((ident, np.array([1.0, 1.0, 0.0], F), np.array([0.0, 0.0, -0.005], F)))
    cases.append((ident, np.array([-1.0, -1.0, 0.0], F), np.array([0.0, 0.0, -0.005], F)))
    return cases


def test_sun_projection_bitwise():
    import shs_gpu
    seen = {"valid": 0, "behind": 0, "w_small": 0, "z_hi": 0, "z_lo": 0, "uv1": 0, "uv0": 0}
    for vp, eye, sun in _sun_cases():
        uv_n, ok_n = np_sun_uv(vp, eye, sun)
        uv_c, ok_c = ref_sun_uv(vp, eye, sun)
        uv_g, ok_g = shs_gpu.Context.light_shafts_sun_uv(vp, eye, sun)
        assert ok_n == ok_c == ok_g, (vp, eye, sun)
        assert uv_n.view(np.uint32).tolist() == uv_c.view(np.uint32).tolist() == uv_g.view(np.uint32).tolist(), (vp, eye, sun)
        # which of the issue's cases this one is (from the numpy version's intermediate values)
        m, p = _f32(vp, 16), (eye + (-sun) * F(100.0)).astype(F)
        w = F(F(F(m[3] * p[0]) + F(m[7] * p[1])) + F(F(m[11] * p[2]) + m[15]))
        z = F(F(F(m[2] * p[0]) + F(m[6] * p[1])) + F(F(m[10] * p[2]) + m[14]))
        seen["valid"] += ok_n
        seen["behind"] += bool(w < 0)
        seen["w_small"] += bool(abs(w) <= F(1e-6))
        if abs(w) > F(1e-6):
            nz = F(z / w)
            seen["z_hi"] += bool(1 < nz <= np.nextafter(F(1), F(2)) + F(1e-5)) and not ok_n
            seen["z_lo"] += bool(-1 - F(1e-5) <= nz < -1) and not ok_n
            seen["uv1"] += bool(ok_n and uv_n[0] == 1 and uv_n[1] == 1)
            seen["uv0"] += bool(ok_n and uv_n[0] == 0 and uv_n[1] == 0)
        else:
            assert not ok_n and uv_n.tolist() == [F(0.5), F(0.2)]
    assert seen["valid"] >= 40 and seen["behind"] >= 40 and seen["w_small"] == 2, seen
    assert seen["z_hi"] >= 1 and seen["z_lo"] >= 1 and seen["uv1"] == 1 and seen["uv0"] == 1, seen


def test_c5_scene_sun_is_behind_the_camera():
    import shs_gpu
    _frame, _draws, vp, eye, sun = _c5_camera()
    for uv_ok in (shs_gpu.Context.light_shafts_sun_uv(vp, eye, sun), ref_sun_uv(vp, eye, sun), np_sun_uv(vp, eye, sun)):
        assert uv_ok[1] is False
    p = (eye + (-sun) * F(100.0)).astype(F)
    w = float(vp[3] * p[0] + vp[7] * p[1] + vp[11] * p[2] + vp[15])
    assert -95 < w < -80, w                          # clip.w ~ -88
    for P, want in (((0, 1.5, 0), (0.50, 0.50)), ((3, 6, 0), (0.60, 0.74)), ((-4, 5, 2), (0.39, 0.69))):
        uv, ok = shs_gpu.Context.light_shafts_sun_uv(vp, eye, _aim(eye, P))
        assert ok and np.allclose(uv, want, atol=0.006), (P, uv)


# ---- CPU 2: the restatement pinned by the numpy version -------------------------------------------
GRID_SIZES = [(352, 200), (97, 61), (64, 64), (37, 1), (1, 29), (1, 1)]
GRID_SUNS = [(0.5, 0.2), (0.0, 1.0), (0.93, 0.07), (1.0, 0.0)]
GRID_PARAMS = [dict(), dict(steps=3), dict(steps=96, density=1.0, decay=1.0, weight=0.02), dict(density=2.5),
               dict(density=1e30), dict(decay=0.5, weight=5.0), dict(weight=-1.0), dict(weight=1e9), dict(weight=1e30)]


@pytest.mark.parametrize("size", GRID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_numpy_version(size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    ldr = _random_ldr(rng, w, h)
    depth = _random_depth(rng, w, h)
    assert w * h < 50 or (np.isnan(depth).any() and np.isinf(depth).any())
    for sun in GRID_SUNS:
        for params in GRID_PARAMS:
            for dp in (None, depth):
                got, gb = ref_shafts_uv(ldr, dp, sun, **params)
                want, wb = np_shafts_uv(ldr, dp, sun, **params)
                assert np.array_equal(gb, wb), (size, sun, params, dp is not None, int((gb != wb).sum()))
                assert np.array_equal(got, want), (size, sun, params, dp is not None)


# ---- CPU 3: hand-computed known answers -----------------------------------------------------------
def test_weight_1e30_wraps_every_boost_to_zero():
    rng = np.random.default_rng(1)
    ldr = _random_ldr(rng, 40, 24)
    out, boost = ref_shafts_uv(ldr, None, (0.5, 0.2), weight=1e30)
    assert not boost.any()
    assert np.array_equal(out[..., :3], ldr[..., :3]) and np.all(out[..., 3] == 255)
    _, b9 = ref_shafts_uv(ldr, None, (0.5, 0.2), weight=1e9)   # the (int)(long) wrap: a 0 / 120 pattern
    assert set(np.unique(b9)) == {0, 120}


def _taps(w, h, sun_uv, steps=48, density=0.8):
    """Per step the tapped texel of every pixel, from the cited lines in float64-free float32."""
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = xs.astype(F) / F(max(1, w - 1)), ys.astype(F) / F(max(1, h - 1))
    for i in range(steps):
        t = F(i) / F(steps)
        sx = _clamp(_lround_int((u + (F(sun_uv[0]) - u) * t * F(density)) * F(w - 1)), 0, w - 1)
        sy = _clamp(_lround_int((v + (F(sun_uv[1]) - v) * t * F(density)) * F(h - 1)), 0, h - 1)
        yield sx, sy


def test_nan_depth_texel_zeroes_exactly_its_rays():
    w, h, sun, tx, ty = 48, 32, (0.5, 0.25), 30, 12
    ldr = np.full((h, w, 4), 200, np.uint8)
    depth = np.full((h, w), 0.75, F)
    params = dict(weight=0.01)
    _, clean = ref_shafts_uv(ldr, depth, sun, **params)
    assert clean.min() > 0 and clean.max() < 120
    depth[ty, tx] = np.nan
    out, hit = ref_shafts_uv(ldr, depth, sun, **params)
    tapped = np.zeros((h, w), bool)
    for sx, sy in _taps(w, h, sun):
        tapped |= (sx == tx) & (sy == ty)
    assert 5 < tapped.sum() < w * h // 4 and tapped[ty, tx]
    assert not hit[tapped].any()
    assert np.array_equal(hit[~tapped], clean[~tapped])
    assert np.array_equal(out[tapped], np.full((int(tapped.sum()), 4), (200, 200, 200, 255), np.uint8))


def test_decay_zero_keeps_the_first_term():
    rng = np.random.default_rng(2)
    w, h = 33, 21
    ldr = _random_ldr(rng, w, h)
    depth = rng.uniform(-0.2, 1.2, size=(h, w)).astype(F)
    weight = F(0.7)
    out, boost = ref_shafts_uv(ldr, depth, (0.3, 0.9), decay=0.0, weight=float(weight))
    rgb = ldr[..., :3].astype(F) / F(255.0)
    luma = (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]
    s = luma * _clamp(depth, F(0.0), F(1.0))        # step 0 taps the pixel itself (t = 0)
    want = _clamp(_lround_int((s * F(1.0) * weight) * F(80.0)), 0, 120)
    assert np.array_equal(boost, want) and len(np.unique(boost)) > 20
    assert np.array_equal(out[..., 0], np.minimum(ldr[..., 0].astype(int) + want, 255))
    assert np.array_equal(out[..., 2], np.minimum(ldr[..., 2].astype(int) + want // 2, 255))


def test_identity_cases():
    rng = np.random.default_rng(3)
    ldr = _random_ldr(rng, 29, 17)
    assert (ldr[..., 3] != 255).any()
    out, boost = ref_shafts_uv(ldr, None, (0.5, 0.2), weight=0.0)
    assert not boost.any() and np.array_equal(out[..., :3], ldr[..., :3]) and np.all(out[..., 3] == 255)
    black = np.zeros((17, 29, 4), np.uint8)
    out, boost = ref_shafts_uv(black, None, (0.5, 0.2), density=0.0)
    assert not boost.any() and not out[..., :3].any() and np.all(out[..., 3] == 255)
    # the whole pass: disabled, or the sun off the screen, leaves every byte (alpha too)
    ident = np.eye(4, dtype=F).reshape(16)
    for kw, sun in ((dict(enable=False), (0.0, 0.0, -0.005)), (dict(), (0.0, 0.0, 0.05))):   # ndc.z = -5
        out, _, ran = ref_shafts(ldr, None, ident, (0, 0, 0), sun, **kw)
        assert not ran and np.array_equal(out, ldr)
    out, boost, ran = ref_shafts(ldr, None, ident, (0, 0, 0), (0.0, 0.0, -0.005))
    assert ran and boost.any()


def test_abi_surface():
    import shs_gpu
    from shs_gpu import _abi
    L = shs_gpu.lib()
    for name in ("shs_light_shafts", "shs_light_shafts_sun_uv"):
        assert getattr(L, name).restype is ctypes.c_int
    assert L.shs_abi_version() == 1
    assert ctypes.sizeof(_abi.LightShaftsDescC) == 4 * (2 + 3 + 3 + 3 + 16 + 1)
    header = open(os.path.join(os.path.dirname(HERE), "include", "shs_gpu.h")).read()
    assert "#define SHS_LIGHT_SHAFTS_NO_DEPTH 1u" in header and _abi.LIGHT_SHAFTS_NO_DEPTH == 1
    assert callable(shs_gpu.Context.light_shafts)


# ---- GPU ------------------------------------------------------------------------------------------
SUN_TARGETS = [(0.0, 1.5, 0.0), (3.0, 6.0, 0.0), (-4.0, 5.0, 2.0)]


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    try:
        yield c
    finally:
        c.close()


def _memcpy_h2d(dst, src):
    hip = ctypes.CDLL("libamdhip64.so.7")   # by SONAME: the runtime already mapped (shs_gpu._abi.load)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert src.flags.c_contiguous
    rc = hip.hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(src.ctypes.data), src.nbytes, 1)   # hipMemcpyHostToDevice
    assert rc == 0, rc


# (name, sun target index or None for the scene's own sun, light_shafts arguments, spread condition)
RENDERED = [("defaults_P0", 0, dict(), True), ("defaults_P1", 1, dict(), True), ("defaults_P2", 2, dict(), True),
            ("weight005", 0, dict(weight=0.05), True), ("weight005_nodepth", 0, dict(weight=0.05, use_depth=False), True),
            ("steps3", 0, dict(steps=3), False), ("steps96", 1, dict(steps=96, density=1.0, decay=1.0, weight=0.02), False),
            ("density25", 2, dict(density=2.5), False), ("disabled", 0, dict(enable=False), False),
            ("scene_sun", None, dict(), False)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", RENDERED, ids=lambda c: c[0])
def test_rendered_frame_exact(ctx, case):
    _name, target, kw, spread = case
    frame, draws, vp, eye, scene_sun = _c5_camera(352, 200)
    sun = scene_sun if target is None else _aim(eye, SUN_TARGETS[target])
    ctx.render_pbr_forward(frame, draws)
    ctx.tonemap(1.0, 2.2)
    base, base_pre = ctx.resolve_ldr()
    _, depth, _ = ctx.resolve_lib()
    ctx.light_shafts(vp, eye, sun, **kw)
    got, pre = ctx.resolve_ldr()
    ref_kw = {k: v for k, v in kw.items() if k != "use_depth"}
    want, boost, ran = ref_shafts(base, depth if kw.get("use_depth", True) else None, vp, eye, sun, **ref_kw)
    if spread:   # a boost that is all 0 or all 120 would show nothing
        assert ran and len(np.unique(boost)) >= 8, np.unique(boost)
        assert ((boost == 0) | (boost == 120)).mean() <= 0.5
    if target is None or not kw.get("enable", True):
        assert not ran and np.array_equal(got, base) and np.array_equal(pre, base_pre)
    else:
        assert ran and not np.array_equal(want, base)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} byte mismatches, first {bad[:4]}"
    assert np.array_equal(pre, got[::-1])


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 40), (97, 61)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_planes_exact(ctx, size):
    """A random LDR (alpha not 255) and a depth plane in [-0.2, 1.2] with NaN and +-inf copied into the
    device targets: the NaN propagation and the integer wrap of huge weights."""
    from shs_gpu import scene_lib
    W, H = size
    frame, draws = scene_lib.c5_scene(W, H)[:2]
    rng = np.random.default_rng(W + H)
    ldr = _random_ldr(rng, W, H)
    depth = _random_depth(rng, W, H, neg_inf=True)
    assert np.isnan(depth).any() and np.isposinf(depth).any() and np.isneginf(depth).any()
    vp, eye = np.eye(4, dtype=F).reshape(16), (0.0, 0.0, 0.0)
    sun = (-0.003, 0.002, -0.005)                    # identity viewproj: sun_uv = (0.65, 0.4)
    for kw in (dict(), dict(weight=1e9), dict(weight=1e30), dict(weight=0.02)):
        ctx.render_pbr_forward(frame, draws)
        ctx.tonemap(1.0, 2.2)
        ctx.synchronize_lib()
        _memcpy_h2d(ctx.ldr_device_targets()[0], ldr)
        _memcpy_h2d(ctx.lib_device_targets()[1], depth)
        ctx.light_shafts(vp, eye, sun, **kw)
        got, pre = ctx.resolve_ldr()
        _, got_depth, _ = ctx.resolve_lib()
        assert np.array_equal(got_depth.view(np.uint32), depth.view(np.uint32)), "injected depth was overwritten"
        want, boost, ran = ref_shafts(ldr, depth, vp, eye, sun, **kw)
        assert ran
        if not kw:             # a NaN tap zeroes a ray that would otherwise saturate
            assert (boost == 0).mean() > 0.2 and (boost == 120).mean() > 0.2
        elif kw["weight"] == 0.02:
            assert len(np.unique(boost)) >= 8 and (boost == 0).mean() > 0.2 and boost.max() < 120
        elif kw["weight"] == 1e9:
            assert set(np.unique(boost)) == {0, 120}
        else:
            assert not boost.any()
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{kw}: {len(bad)} byte mismatches, first {bad[:4]}"
        assert np.array_equal(pre, got[::-1])


@pytest.mark.gpu
def test_tiny_sizes_in_one_context(oracle_mod):
    """max(1, w - 1) denominators, single rows / columns, 1x1, and the mask plane resized with the frame,
    the fused and the separate tonemap in turn."""
    import shs_gpu
    with shs_gpu.Context(0) as c:
        for i, (W, H) in enumerate([(96, 64), (1, 1), (37, 1), (1, 29), (17, 9), (96, 64)]):
            frame, draws, vp, eye, _ = _c5_camera(W, H)
            sun = _aim(eye, SUN_TARGETS[0])           # the look-at centre: on the screen at every aspect
            fused = i % 2 == 0
            c.fuse_tonemap(1.3, 2.2, ldr=True, present=True, enable=fused)
            c.render_pbr_forward(frame, draws)
            if not fused:
                c.tonemap(1.3, 2.2, ldr=True, present=True)
            c.light_shafts(vp, eye, sun, weight=0.05)
            got, pre = c.resolve_ldr()
            hdr, depth, _ = c.resolve_lib()
            base, _ = oracle_mod.tonemap(hdr, 1.3, 2.2)
            want, boost, ran = ref_shafts(base, depth, vp, eye, sun, weight=0.05)
            assert ran and (W * H < 100 or boost.any()), (W, H)
            assert np.array_equal(got, want), (W, H, fused)
            assert np.array_equal(pre, got[::-1]), (W, H, fused)
        c.fuse_tonemap(enable=False)


@pytest.mark.gpu
def test_chain_order(ctx, oracle_mod):
    frame, draws, vp, eye, _ = _c5_camera(352, 200)
    sun = _aim(eye, SUN_TARGETS[0])
    ctx.render_pbr_forward(frame, draws)
    ctx.tonemap(1.0, 2.2)
    base, _ = ctx.resolve_ldr()
    ctx.light_shafts(vp, eye, sun, weight=0.05)
    ctx.motion_blur(min_velocity_px=0.0)
    blurred, _ = ctx.resolve_motion_blur()
    shafted, pre = ctx.resolve_ldr()
    _, depth, motion = ctx.resolve_lib()
    want, _, ran = ref_shafts(base, depth, vp, eye, sun, weight=0.05)
    assert ran and not np.array_equal(want, base)
    assert np.array_equal(shafted, want) and np.array_equal(pre, want[::-1])
    assert np.array_equal(blurred, oracle_mod.motion_blur(want, depth, motion, min_velocity_px=0.0))
    assert not np.array_equal(blurred, oracle_mod.motion_blur(base, depth, motion, min_velocity_px=0.0))
    ctx.tonemap(1.0, 2.2)                             # a new tonemap starts over
    again, _ = ctx.resolve_ldr()
    assert np.array_equal(again, base)


# The re-issue scene of tests/test_lib_history.py::test_spill_overflow_reissue, built here: ten stacks of
# 8,000 small triangles, each inside its own 32x32 bin tile of a 256x192 frame, plus 600 padding
# triangles: 10 * (8,000 - 256) = 77,440 spilled entries against the initial 65,536.
RW, RH, RT, TEN_N = 256, 192, 32, 8000
TEN_CENTRES = [(RT * tx + RT // 2, RT * ty + RT // 2) for ty in (1, 4) for tx in range(5)]


def _tris(rng, cx, cy, spread, n):
    c = np.stack([cx + rng.uniform(-spread[0], spread[0], n), cy + rng.uniform(-spread[1], spread[1], n)], axis=1)
    r = rng.uniform(2.0, 3.0, n)
    a = rng.uniform(0.0, 2.0 * np.pi, n)[:, None] + np.arange(3)[None, :] * (2.0 * np.pi / 3.0)
    px = c[:, None, :] + r[:, None, None] * np.stack([np.cos(a), np.sin(a)], axis=2)
    z = np.float32([-0.5, 0.0, 0.5])[rng.integers(0, 3, n)]
    pos = np.empty((n, 3, 3), F)
    pos[..., 0] = px[..., 0] * (2.0 / RW) - 1.0
    pos[..., 1] = px[..., 1] * (2.0 / RH) - 1.0
    pos[..., 2] = z[:, None]
    pos = pos.reshape(-1, 3)
    return pos, rng.normal(size=pos.shape).astype(F)


def _ten_stacks():
    from shs_gpu.lib_path import LibDraw, LibFrame, LibMesh
    rng = np.random.default_rng(77)
    parts = [_tris(rng, cx, cy, (6.0, 6.0), TEN_N) for cx, cy in TEN_CENTRES]
    stacks = LibMesh(np.concatenate([p for p, _ in parts]), np.concatenate([n for _, n in parts]))
    pad = LibMesh(*_tris(rng, 0.85 * RW, 0.5 * RH, (0.1 * RW - 3.0, 0.45 * RH), 600))
    frame = LibFrame(RW, RH, depth_motion=True, zn=1.0, zf=1.0, bg_gradient=False, clear_hdr=(0.1, 0.2, 0.3, 1.0))
    return frame, [LibDraw(mesh=pad, program=2, cull_mode=0), LibDraw(mesh=stacks, program=2, cull_mode=0)]


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
def test_reissued_camera_pass_replays_the_chain(oracle_mod, fused):
    """The first camera pass of a fresh context overflows the spill capacity; the render, the tonemap
    and the light shafts are all enqueued before anything is resolved, so the shafts first ran on an
    incomplete frame: the re-issue must replay tonemap then shafts, once."""
    import shs_gpu
    frame, draws = _ten_stacks()
    vp, eye, sun = np.eye(4, dtype=F).reshape(16), (0.0, 0.0, 0.0), (-0.003, -0.004, -0.002)   # sun_uv (0.65, 0.7)
    kw = dict(weight=0.02)
    with shs_gpu.Context(0) as c:
        c.enable_timing(True)
        c.lib_timing_reset()
        c.fuse_tonemap(1.0, 2.2, ldr=True, present=True, enable=fused)
        c.render_pbr_forward(frame, draws)
        if not fused:
            c.tonemap(1.0, 2.2, ldr=True, present=True)
        c.light_shafts(vp, eye, sun, **kw)
        got, pre = c.resolve_ldr()
        n_pass, _ = c.lib_timing_read()
        assert n_pass["camera"] == 2, n_pass
        hdr, depth, _ = c.resolve_lib()
        c.fuse_tonemap(enable=False)
    base, _ = oracle_mod.tonemap(hdr, 1.0, 2.2)
    want, boost, ran = ref_shafts(base, depth, vp, eye, sun, **kw)
    assert ran and len(np.unique(boost)) >= 8 and boost.max() < 120
    twice, _, _ = ref_shafts(want, depth, vp, eye, sun, **kw)
    assert not np.array_equal(twice, want) and not np.array_equal(want, base)
    assert np.array_equal(got, want)
    assert np.array_equal(pre, got[::-1])


@pytest.mark.gpu
def test_validation():
    import shs_gpu
    from shs_gpu import ShsError
    frame, draws, vp, eye, _ = _c5_camera(96, 64)
    sun = _aim(eye, SUN_TARGETS[0])
    with shs_gpu.Context(0) as c:
        c.render_pbr_forward(frame, draws)
        with pytest.raises(ShsError):
            c.light_shafts(vp, eye, sun)              # no tonemap yet
        c.tonemap(ldr=False, present=True)
        with pytest.raises(ShsError):
            c.light_shafts(vp, eye, sun)              # the tonemap wrote no RT_ColorLDR
        c.tonemap()
        with pytest.raises(ShsError):
            c.light_shafts(vp, eye, sun, steps=1025)
        with pytest.raises(ShsError):
            c.light_shafts(vp, eye, sun, density=float("nan"))
        base, _ = c.resolve_ldr()
        c.light_shafts(vp, eye, sun, steps=1024, weight=0.01)   # the largest accepted step count
        assert not np.array_equal(c.resolve_ldr()[0], base)
        with pytest.raises(ShsError):
            c.light_shafts(vp, eye, sun)              # once per tonemap
        frame.shard_rank, frame.shard_count = 0, 3
        c.render_pbr_forward(frame, draws)
        c.tonemap()
        with pytest.raises(ShsError):
            c.light_shafts(vp, eye, sun)              # a tile-sharded frame
