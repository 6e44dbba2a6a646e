"""The reference of the Toon, Gooch, Oren-Nayar, normal- and depth-visualiser shading models
(tests/legacy_shaders_ref/ref_legacy_shaders.c, a line-cited C restatement of the four demos) and what pins
it on the CPU:

1. its raster against the oracle every other legacy test trusts: depth and coverage bit for bit, and its own
   Blinn-Phong FS (the split-screen demo's centre pane) byte for byte and float for float;
2. its five FS against an independent float32 numpy version, over random varyings and the edge cases;
3. the share of pixels the GPU tests may excuse, per frame they use: at most 0.5 % of the covered ones.

tests/test_legacy_shaders.py (GPU) imports the wrapper, the scenes and the edge cases from here."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import helpers

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "legacy_shaders_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_legacy_shaders_ref.so")
F = np.float32
INF = np.float32(np.inf)
BLINN, TOON, GOOCH, OREN, NORMAL_VIS, DEPTH_VIS = 3, 4, 5, 6, 7, 8
NEW_MODELS = (TOON, GOOCH, OREN, NORMAL_VIS, DEPTH_VIS)
W, H = 160, 120                     # two by two 80x80 tile jobs
CAP = 0.005                         # excusable pixels per frame: 0.5 % of the covered ones
COS_BETA_MIN = 2.0 ** -7            # Oren-Nayar pixels below it are left out (tan(beta) amplifies acosf's ulp)
_P = ctypes.c_void_p
_ref = None


class RefDraw(ctypes.Structure):
    _fields_ = [("positions", _P), ("normals", _P), ("n_tris", ctypes.c_int32), ("shading", ctypes.c_int32),
                ("mvp", ctypes.c_float * 16), ("model", ctypes.c_float * 16), ("light_dir", ctypes.c_float * 3),
                ("camera_pos", ctypes.c_float * 3), ("color", ctypes.c_uint8 * 4)]


def ref_lib():
    global _ref
    if _ref is None:
        subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
        L = ctypes.CDLL(REF_LIB)
        L.rls_render.restype = ctypes.c_int
        L.rls_render.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(RefDraw), ctypes.c_int] + [_P] * 6
        L.rls_shade_samples.restype = ctypes.c_int
        L.rls_shade_samples.argtypes = [ctypes.POINTER(RefDraw), ctypes.c_int] + [_P] * 7
        _ref = L
    return _ref


def _fill_uniforms(a, shading, mvp, model, light_dir, camera_pos, color):
    a.shading = int(shading)
    for k in range(16):
        a.mvp[k], a.model[k] = float(mvp[k]), float(model[k])
    for k in range(3):
        a.light_dir[k], a.camera_pos[k] = float(light_dir[k]), float(camera_pos[k])
    for k in range(4):
        a.color[k] = int(color[k])


def ref_render(width, height, draws, tile=(80, 80), shading_of=None):
    """draws: shs_gpu.Draw list (host meshes) -> dict of planes: color, depth, prequant, spec_margin,
    cos_beta, draw_id (canvas rows but depth).  shading_of: per draw the model the reference shades it with
    (a Flat .. Phong draw rasters the same whatever shades it)."""
    arr = (RefDraw * max(len(draws), 1))()
    keep = []
    for i, d in enumerate(draws):
        pos = np.ascontiguousarray(d.mesh.positions, F)
        nrm = np.ascontiguousarray(d.mesh.normals, F)
        keep += [pos, nrm]
        arr[i].positions, arr[i].normals, arr[i].n_tris = pos.ctypes.data, nrm.ctypes.data, pos.shape[0]
        _fill_uniforms(arr[i], d.shading if shading_of is None else shading_of[i], d.mvp, d.model, d.light_dir,
                       d.camera_pos, d.color)
    out = {"color": np.empty((height, width, 4), np.uint8), "depth": np.empty((height, width), F),
           "prequant": np.empty((height, width, 4), F), "spec_margin": np.empty((height, width), F),
           "cos_beta": np.empty((height, width), F), "draw_id": np.empty((height, width), np.int32)}
    rc = ref_lib().rls_render(width, height, tile[0], tile[1], arr, len(draws), *[out[k].ctypes.data for k in (
        "color", "depth", "prequant", "spec_margin", "cos_beta", "draw_id")])
    assert rc == 0
    return out


def ref_samples(shading, light_dir, camera_pos, color, normal_sum, world_pos, clip_z):
    ns = np.ascontiguousarray(np.asarray(normal_sum, F).reshape(-1, 3))
    wp = np.ascontiguousarray(np.asarray(world_pos, F).reshape(-1, 3))
    cz = np.ascontiguousarray(np.asarray(clip_z, F).reshape(-1))
    n = ns.shape[0]
    u = RefDraw()
    _fill_uniforms(u, shading, np.zeros(16), np.zeros(16), light_dir, camera_pos, color)
    out = {"rgba": np.zeros((n, 4), np.uint8), "prequant": np.zeros((n, 4), F), "spec_margin": np.zeros(n, F),
           "cos_beta": np.zeros(n, F)}
    rc = ref_lib().rls_shade_samples(ctypes.byref(u), n, ns.ctypes.data, wp.ctypes.data, cz.ctypes.data,
                                     *[out[k].ctypes.data for k in ("rgba", "prequant", "spec_margin", "cos_beta")])
    assert rc == 0
    return out


# ---- the scenes -----------------------------------------------------------------------------------------
LIGHT = (-1.0, -0.4, 1.0)
COLOR = (60, 100, 200, 255)
CAM = (0.0, 5.0, -20.0)


def monkey_draw(shading, position=(0.0, 0.0, 10.0), scale=4.0, rotation=-30.0, cam_pos=CAM, yaw=0.0, pitch=0.0):
    """One Suzanne of the C1 scene at model yaw -30 (the Toon / Oren-Nayar demos' rotation_angle) under the
    light normalize(-1, -0.4, 1); Flat takes its own uniforms (scene.make_draw)."""
    from shs_gpu import scene
    view, proj = scene.camera(cam_pos, yaw, pitch)
    model = scene.model_trs(position, rotation, (scale, scale, scale))
    return scene.make_draw(scene.monkey(), shading, model, view, proj, scene.glm_normalize(LIGHT), cam_pos, COLOR)


def frame_desc(**kw):
    import shs_gpu
    return shs_gpu.Frame(W, H, prequant=True, **kw)


@functools.lru_cache(maxsize=None)
def model_frame(shading):
    """The frame of one model: (draws, the reference's planes)."""
    draws = [monkey_draw(shading)]
    return draws, ref_render(W, H, draws)


MIXED_POS = [((i - 4) * 1.6, (i % 2) * 0.8 - 0.4, 10.0 + (i * 5) % 9 * 0.5) for i in range(9)]


@functools.lru_cache(maxsize=None)
def mixed_frame():
    """Nine overlapping Suzannes, one per model 0..8: (draws, the reference's planes with draws 0..2 shaded as
    Blinn-Phong -- the winner plane says which pixels are its to judge)."""
    draws = [monkey_draw(m, position=MIXED_POS[m], scale=2.5) for m in range(9)]
    return draws, ref_render(W, H, draws, shading_of=[max(m, BLINN) for m in range(9)])


POSES = [dict(cam_pos=(0.0, 5.0, -20.0)), dict(cam_pos=(3.0, 4.0, -19.0), yaw=6.0), dict(cam_pos=(-4.0, 6.0, -18.0), yaw=-9.0),
         dict(cam_pos=(1.0, 2.0, -22.0), pitch=5.0), dict(cam_pos=(-2.0, 7.0, -21.0), yaw=-4.0, pitch=-6.0)]


def excusable(shading, planes):
    """The pixels (or samples) a GPU test may leave out: a Toon specular step within TOL of its threshold, an
    Oren-Nayar fragment whose cos(beta) is below 2^-7."""
    if shading == TOON:
        return planes["spec_margin"] <= F(helpers.TOL)
    if shading == OREN:
        return planes["cos_beta"] < F(COS_BETA_MIN)
    return np.zeros(planes["spec_margin"].shape, bool)


def covered(planes):
    return planes["depth"][::-1] < helpers.FLT_MAX   # canvas rows


# ---- the edge cases of the sample tests -----------------------------------------------------------------
EDGE_LIGHT = (0.0, 0.0, -1.0)       # L = normalize(-light_dir) = (0, 0, 1)
EDGE_CAM = (0.0, -10.0, 0.0)        # V = (0, -1, 0) at the origin


def _bisect_flip(shading, make, lo, hi):
    """Two parameters a float64 bisection can no longer separate, whose samples the reference shades
    differently: the inputs either side of one of the shader's comparisons."""
    def out(t):
        ns, wp = make(t)
        return ref_samples(shading, EDGE_LIGHT, EDGE_CAM, COLOR, [ns], [wp], [0.0])["rgba"][0].tobytes()
    a, b = out(lo), out(hi)
    assert a != b, "the bracket does not hold a decision"
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if out(mid) == a:
            lo = mid
        else:
            hi = mid
    return lo, hi


@functools.lru_cache(maxsize=None)
def toon_threshold_samples():
    """(normal_sum [n, 3], world_pos [n, 3]): for NdotL = 0.95, 0.5, 0.3 (the rim's), 0.25 and rimDot = 0.7
    the two samples either side, found by bisecting the normal's angle against the reference."""
    ns, wp = [], []

    def sweep_l(t):   # N.L = cos t, V.N = 0 (rimDot = 1: the rim follows NdotL > 0.3)
        return (np.sin(t), 0.0, np.cos(t)), (0.0, 0.0, 0.0)

    def sweep_v(t):   # V.N = sin t, N.L = cos t ~ 0.954
        return (0.0, -np.sin(t), np.cos(t)), (0.0, 0.0, 0.0)

    for thr in (0.95, 0.5, 0.3, 0.25):
        t0 = float(np.arccos(thr))
        for t in _bisect_flip(TOON, sweep_l, t0 - 2e-3, t0 + 2e-3):
            a, b = sweep_l(t)
            ns.append(a), wp.append(b)
    t0 = float(np.arcsin(0.3))       # rimDot = 1 - V.N = 0.7
    for t in _bisect_flip(TOON, sweep_v, t0 - 2e-3, t0 + 2e-3):
        a, b = sweep_v(t)
        ns.append(a), wp.append(b)
    return np.asarray(ns, F), np.asarray(wp, F)


def toon_specular_samples():
    """Normals a few degrees off the halfway vector of L = (0, 0, 1) and V = (0, -1, 0): pow(NdotH, 32) passes
    0.5 near 11.9 degrees."""
    h = np.array([0.0, -1.0, 1.0]) / np.sqrt(2.0)
    side = np.array([1.0, 0.0, 0.0])
    ang = np.radians(np.linspace(0.0, 25.0, 101))
    ns = np.cos(ang)[:, None] * h + np.sin(ang)[:, None] * side
    return ns.astype(F), np.zeros((ang.size, 3), F)


OREN_CAM = (0.0, 0.0, 5.0)
OREN_EDGE = {   # name: (normal_sum, world_pos) under L = (0, 0, 1), camera (0, 0, 5)
    "V parallel to N (NaN)": ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0)),
    "V parallel to N, longer sum": ((0.0, 0.0, 2.5), (0.0, 0.0, -3.0)),
    "NdotL = 0 and NdotV = 0": ((1.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    "NdotL = 0": ((0.0, 1.0, 0.0), (0.0, -5.0, 5.0)),
    "NdotV = 0, N.L = 1": ((0.0, 0.0, 1.0), (3.0, 0.0, 5.0)),
    "N.L = 1, V oblique": ((0.0, 0.0, 1.0), (1.0, 2.0, 0.0)),
    "oblique": ((0.3, -0.2, 0.8), (1.0, 2.0, 0.0)),
}
DEPTH_EDGE = np.array([-1.0, 0.0, 40.0, np.nextafter(F(40.0), F(0.0)), 1e9, np.nan, 13.7], F)


def random_varyings(n, seed):
    rng = np.random.default_rng(seed)
    ns = rng.normal(size=(n, 3)).astype(F) * rng.uniform(0.3, 1.2, size=(n, 1)).astype(F)
    wp = rng.uniform(-6.0, 6.0, size=(n, 3)).astype(F)
    cz = rng.uniform(-5.0, 60.0, size=n).astype(F)
    return ns, wp, cz


def edge_sets():
    """model -> list of (light_dir, camera_pos, normal_sum, world_pos, clip_z) sample sets."""
    tn, tw = toon_threshold_samples()
    sn, sw = toon_specular_samples()
    on = np.asarray([v[0] for v in OREN_EDGE.values()], F)
    ow = np.asarray([v[1] for v in OREN_EDGE.values()], F)
    z = lambda a: np.zeros(a.shape[0], F)
    return {
        TOON: [(EDGE_LIGHT, EDGE_CAM, tn, tw, z(tn)), (EDGE_LIGHT, EDGE_CAM, sn, sw, z(sn))],
        GOOCH: [(EDGE_LIGHT, EDGE_CAM, sn, sw, z(sn))],
        OREN: [(EDGE_LIGHT, OREN_CAM, on, ow, z(on))],
        NORMAL_VIS: [(EDGE_LIGHT, EDGE_CAM, np.vstack([np.zeros((1, 3), F), sn[:5]]), np.zeros((6, 3), F), np.zeros(6, F))],
        DEPTH_VIS: [(EDGE_LIGHT, EDGE_CAM, np.ones((DEPTH_EDGE.size, 3), F), np.zeros((DEPTH_EDGE.size, 3), F), DEPTH_EDGE)],
    }


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- float32 numpy version of the five FS (independent of the C text) ---------------------------------------
def _gmax(x, y):
    return np.where(x < y, y, x)


def _gmin(x, y):
    return np.where(y < x, y, x)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    return v * (F(1.0) / np.sqrt(_dot(v, v)))[..., None]


def _f64(fn, *x):
    """A libm call of the shader, in float64 and rounded once to float32."""
    return fn(*[np.asarray(v, np.float64) for v in x]).astype(F)


def numpy_fs(shading, light_dir, camera_pos, color, normal_sum, world_pos, clip_z):
    """-> (pre-truncation floats [n, 3], bytes [n, 3]) of the reference FS lines, vectorised."""
    with np.errstate(all="ignore"):
        ns, wp, cz = np.asarray(normal_sum, F), np.asarray(world_pos, F), np.asarray(clip_z, F)
        if shading == DEPTH_VIS:
            vis = F(1.0) - _gmin(_gmax(cz / F(40.0), F(0.0)), F(1.0))
            pre = np.repeat((vis * F(255.0))[:, None], 3, axis=1)
        else:
            norm = _normalize(_normalize(ns))        # draw_triangle_tile's, then the FS's
            if shading == NORMAL_VIS:
                pre = ((norm + F(1.0)) * F(0.5)) * F(255.0)
            else:
                L = _normalize(-np.asarray(light_dir, F))
                V = _normalize(np.asarray(camera_pos, F) - wp)
                oc = np.asarray(color[:3], F) / F(255.0)
                Hh = _normalize(L + V)
                ndh = _gmax(_dot(norm, Hh), F(0.0))
                if shading == TOON:
                    ndl = _gmax(_dot(norm, L), F(0.0))
                    inten = np.where(ndl > F(0.95), F(1.0), np.where(ndl > F(0.5), F(0.7), np.where(ndl > F(0.25), F(0.4), F(0.2))))
                    spec = np.where(_f64(np.power, ndh, 32.0) > F(0.5), F(0.8), F(0.0))
                    rim_dot = F(1.0) - _gmax(_dot(V, norm), F(0.0))
                    rim = np.where((rim_dot > F(0.7)) & (ndl > F(0.3)), F(0.5), F(0.0))
                    res = (oc * inten[:, None] + spec[:, None]) + rim[:, None]
                elif shading == GOOCH:
                    t = (_dot(norm, L) + F(1.0)) / F(2.0)
                    cool = np.array([0.0, 0.0, 0.55], F) + F(0.25) * oc
                    warm = np.array([0.6, 0.6, 0.1], F) + F(0.25) * oc
                    res = t[:, None] * warm + (F(1.0) - t)[:, None] * cool
                    res = res + ((F(1.0) * _f64(np.power, ndh, 32.0)) * F(0.7))[:, None]
                else:
                    s2 = F(0.9) * F(0.9)
                    A = F(1.0) - F(0.5) * (s2 / (s2 + F(0.33)))
                    B = F(0.45) * (s2 / (s2 + F(0.09)))
                    ndl = _gmax(_dot(norm, L), F(0.0))
                    ndv = _gmax(_dot(norm, V), F(0.0))
                    tl, tv = _f64(np.arccos, ndl), _f64(np.arccos, ndv)
                    alpha, beta = _gmax(tl, tv), _gmin(tl, tv)
                    vp = _normalize(V - norm * ndv[:, None])
                    lp = _normalize(L - norm * ndl[:, None])
                    cphi = _gmax(_dot(vp, lp), F(0.0))
                    on = ndl * (A + (((B * cphi) * _f64(np.sin, alpha)) * _f64(np.tan, beta)))
                    res = oc * (F(0.15) + on)[:, None]
                pre = _gmin(_gmax(res, F(0.0)), F(1.0)) * F(255.0)
        pre = pre.astype(F)
        by = np.where(np.isnan(pre), 0, pre).astype(np.int32).astype(np.uint8)   # the x86 convert: NaN -> byte 0
    return pre, by


# ---- CPU tests ----------------------------------------------------------------------------------------------
def test_reference_raster_and_blinn_phong_equal_the_oracle(oracle_mod):
    draws = [monkey_draw(BLINN)]
    ref = ref_render(W, H, draws)
    ora_c, ora_d, ora_pq = oracle_mod.render_legacy(W, H, draws, prequant=True)
    assert int(covered(ref).sum()) > 400
    helpers.assert_depth_bitexact(ref["depth"], ora_d)
    assert np.array_equal(ref["color"], ora_c)
    assert np.array_equal(ref["prequant"].view(np.uint32), ora_pq.view(np.uint32))
    # every model rasters the same pixels at the same depth: only the FS differs
    for m in NEW_MODELS:
        helpers.assert_depth_bitexact(model_frame(m)[1]["depth"], ora_d)
        assert np.array_equal(model_frame(m)[1]["color"][..., 3], ora_c[..., 3])
    # and the mixed frame's raster, with its Flat .. Phong draws, is the oracle's
    mdraws, mref = mixed_frame()
    import copy
    sub = [copy.copy(d) for d in mdraws]
    for d in sub[4:]:
        d.shading = BLINN
    mc, md, _ = oracle_mod.render_legacy(W, H, sub)
    helpers.assert_depth_bitexact(mref["depth"], md)
    assert np.array_equal(mref["color"][..., 3], mc[..., 3])
    assert sorted(set(np.unique(mref["draw_id"])) - {-1}) == list(range(9)), "every model wins pixels of the mixed frame"


def test_reference_shaders_equal_the_numpy_version():
    ns, wp, cz = random_varyings(3000, 7)
    for m in NEW_MODELS:
        sets = [(np.asarray(LIGHT, F), CAM, ns, wp, cz)] + edge_sets()[m]
        for light, cam, a, b, c in sets:
            ref = ref_samples(m, light, cam, COLOR, a, b, c)
            pre, by = numpy_fs(m, light, cam, COLOR, a, b, c)
            assert np.array_equal(np.isnan(pre), np.isnan(ref["prequant"][:, :3])), m
            ok = ~np.isnan(pre)
            err = np.abs(pre[ok].astype(np.float64) - ref["prequant"][:, :3][ok])
            # (a Toon sample within an ulp of the specular step may take the other side in numpy's pow)
            if m == TOON:
                keep = ref["spec_margin"] > F(helpers.TOL)
                err = np.abs(pre[keep].astype(np.float64) - ref["prequant"][keep, :3])
                err = err[~np.isnan(err)]
                assert np.array_equal(by[keep], ref["rgba"][keep, :3]), m
            else:
                assert np.array_equal(by, ref["rgba"][:, :3]), m
            assert err.size == 0 or err.max() <= helpers.TOL * 255.0, (m, err.max())
            assert (ref["rgba"][:, 3] == 255).all() and (ref["prequant"][:, 3] == 1.0).all()


def test_reference_edge_cases_are_what_the_shaders_say():
    e = edge_sets()
    # Oren-Nayar, V parallel to N: NaN floats, and the x86 convert makes byte 0 of a NaN
    light, cam, a, b, c = e[OREN][0]
    ref = ref_samples(OREN, light, cam, COLOR, a, b, c)
    assert np.isnan(ref["prequant"][0, :3]).all() and ref["rgba"][0].tolist() == [0, 0, 0, 255]
    assert np.isnan(ref["prequant"][1, :3]).all() and ref["rgba"][1].tolist() == [0, 0, 0, 255]
    assert ref["cos_beta"][2] == 0.0 and np.isfinite(ref["prequant"][6]).all()
    # the depth visualiser: z <= 0 white, z >= 40 black, the float below 40 still black after truncation, NaN byte 0
    light, cam, a, b, c = e[DEPTH_VIS][0]
    ref = ref_samples(DEPTH_VIS, light, cam, COLOR, a, b, c)
    mid = int((F(1.0) - F(13.7) / F(40.0)) * F(255.0))   # 167
    assert ref["rgba"][:, 0].tolist() == [255, 255, 0, 0, 0, 0, mid]
    assert np.isnan(ref["prequant"][5, 0])
    # the normal visualiser of a zero sum: NaN, byte 0
    light, cam, a, b, c = e[NORMAL_VIS][0]
    ref = ref_samples(NORMAL_VIS, light, cam, COLOR, a, b, c)
    assert np.isnan(ref["prequant"][0, :3]).all() and ref["rgba"][0].tolist() == [0, 0, 0, 255]
    # Toon: each pair of threshold samples is shaded differently, and both specular sides are there
    tn, tw = toon_threshold_samples()
    ref = ref_samples(TOON, EDGE_LIGHT, EDGE_CAM, COLOR, tn, tw, np.zeros(tn.shape[0], F))
    assert tn.shape[0] == 10
    for k in range(0, 10, 2):
        assert ref["rgba"][k].tolist() != ref["rgba"][k + 1].tolist()
    sn, sw = toon_specular_samples()
    ref = ref_samples(TOON, EDGE_LIGHT, EDGE_CAM, COLOR, sn, sw, np.zeros(sn.shape[0], F))
    clear = ref["spec_margin"] > F(helpers.TOL)
    on = ref["rgba"][:, 0] >= 204          # + 0.8
    assert (clear & on).sum() > 10 and (clear & ~on).sum() > 10


def test_excusable_pixels_stay_under_the_cap():
    for m in (TOON, OREN):
        planes = model_frame(m)[1]
        n = int(covered(planes).sum())
        assert int((excusable(m, planes) & covered(planes)).sum()) <= CAP * n, m
    _, mref = mixed_frame()
    for m in (TOON, OREN):
        mine = mref["draw_id"] == m
        assert int((excusable(m, mref) & mine).sum()) <= CAP * int(mine.sum()), m
    for k, pose in enumerate(POSES):
        m = NEW_MODELS[k]
        planes = ref_render(W, H, [monkey_draw(m, **pose)])
        n = int(covered(planes).sum())
        assert n > 200 and int((excusable(m, planes) & covered(planes)).sum()) <= CAP * n, (m, k)


def test_constants_and_bindings():
    import shs_gpu
    from shs_gpu import _abi
    assert (shs_gpu.SHADING_TOON, shs_gpu.SHADING_GOOCH, shs_gpu.SHADING_OREN_NAYAR, shs_gpu.SHADING_NORMAL_VIS,
            shs_gpu.SHADING_DEPTH_VIS) == NEW_MODELS
    assert _abi.SHADING_NAMES["oren_nayar"] == OREN and len(_abi.SHADING_NAMES) == 9
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "shs_gpu.h")).read()
    for name, v in (("TOON", 4), ("GOOCH", 5), ("OREN_NAYAR", 6), ("NORMAL_VIS", 7), ("DEPTH_VIS", 8)):
        assert f"#define SHS_SHADING_{name} {v} " in hdr
    L = shs_gpu.lib()
    assert hasattr(L, "shs_legacy_shade_samples")
    assert L.shs_legacy_shade_samples(None, None, 0, None, None, None, None, None) == _abi.SHS_ERR_INVALID
