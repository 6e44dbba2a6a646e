"""The reference of the texture-mapping pipeline, SHADING_TEXTURED (tests/legacy_texture_ref/
ref_legacy_texture.c, a line-cited C restatement of hello_pipeline_texture_mapping.cpp and sample_nearest),
and what pins it on the CPU before anything trusts it:

1. with equal w at all three corners (an orthographic-style mvp whose last row is (0, 0, 0, 1)) the
   perspective-correct sums are the affine ones over invw_sum = (u + v) + w, one or two ulps from 1: coverage
   and the texture-less colour bytes equal oracle.render_legacy's Blinn-Phong frame, depth within those ulps;
2. its sampler against a numpy version, and known answers: a 1x1 texture, u (w - 1) exactly on .5 for even
   and odd texels, uv < 0, uv > 1, NaN;
3. its raster against a float32 numpy per-pixel restatement on a two-triangle scene, with and without a
   texture, with and without UVs;
4. what the GPU tests' scenes cover at 160x120.

tests/test_legacy_texture.py (GPU) imports the wrapper, the scenes and the edge sets from here."""
import copy
import ctypes
import functools
import os
import subprocess

import numpy as np

import helpers

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "legacy_texture_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_legacy_texture_ref.so")
F = np.float32
TEXTURED, BLINN = 9, 3
W, H = 160, 120                     # two by two 80x80 tile jobs
LIGHT = (-1.0, -0.4, 1.0)
COLOR = (200, 200, 200, 255)        # texture_mapping.cpp:171
CAM = (0.0, 5.0, -20.0)
_P = ctypes.c_void_p
_ref = None


class RefDraw(ctypes.Structure):
    _fields_ = [("positions", _P), ("normals", _P), ("uvs", _P), ("n_tris", ctypes.c_int32),
                ("mvp", ctypes.c_float * 16), ("model", ctypes.c_float * 16), ("light_dir", ctypes.c_float * 3),
                ("camera_pos", ctypes.c_float * 3), ("color", ctypes.c_uint8 * 4), ("texels", _P),
                ("tw", ctypes.c_int32), ("th", ctypes.c_int32)]


def ref_lib():
    global _ref
    if _ref is None:
        subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
        L = ctypes.CDLL(REF_LIB)
        L.rlt_render.restype = ctypes.c_int64
        L.rlt_render.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(RefDraw), ctypes.c_int] + [_P] * 5
        L.rlt_sample_nearest.restype = ctypes.c_int
        L.rlt_sample_nearest.argtypes = [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]
        _ref = L
    return _ref


class Tex:
    """A Texture2D as the host's loader leaves it: rgba uint8 [h, w, 4], texel (x, y) at rgba[y, x]."""

    def __init__(self, rgba):
        self.rgba = np.ascontiguousarray(rgba, np.uint8)
        assert self.rgba.ndim == 3 and self.rgba.shape[2] == 4


class SoupMesh:
    def __init__(self, positions, normals, uvs=None):
        self.positions = np.ascontiguousarray(positions, F).reshape(-1, 9)
        self.normals = np.ascontiguousarray(normals, F).reshape(-1, 9)
        self.uvs = None if uvs is None else np.ascontiguousarray(uvs, F).reshape(-1, 6)


def texture_of(draw):
    """The draw's Tex, or None: albedo_tex 0 is the id of "no texture" (a draw list whose albedo_tex are all None
    goes through the untextured render call, which does not take SHADING_TEXTURED)."""
    t = getattr(draw, "albedo_tex", None)
    return None if t is None or (isinstance(t, int) and t == 0) else t


def ref_render(width, height, draws, tile=(80, 80)):
    """draws: shs_gpu.Draw list of SHADING_TEXTURED draws (host meshes, albedo_tex a Tex, 0 or None) -> dict of
    planes: color, prequant, draw_id, texel (canvas rows), depth (screen rows), and `skipped`, the
    fragments invw_sum <= 0 dropped."""
    arr = (RefDraw * max(len(draws), 1))()
    keep = []
    for i, d in enumerate(draws):
        assert d.shading == TEXTURED
        pos = np.ascontiguousarray(d.mesh.positions, F)
        nrm = np.ascontiguousarray(d.mesh.normals, F)
        uvs = getattr(d.mesh, "uvs", None)
        keep += [pos, nrm]
        a = arr[i]
        a.positions, a.normals, a.n_tris = pos.ctypes.data, nrm.ctypes.data, pos.shape[0]
        if uvs is not None:
            uvs = np.ascontiguousarray(uvs, F)
            keep.append(uvs)
            a.uvs = uvs.ctypes.data
        for k in range(16):
            a.mvp[k], a.model[k] = float(d.mvp[k]), float(d.model[k])
        for k in range(3):
            a.light_dir[k], a.camera_pos[k] = float(d.light_dir[k]), float(d.camera_pos[k])
        for k in range(4):
            a.color[k] = int(d.color[k])
        tex = texture_of(d)
        if tex is not None:
            keep.append(tex.rgba)
            a.texels, a.tw, a.th = tex.rgba.ctypes.data, tex.rgba.shape[1], tex.rgba.shape[0]
    out = {"color": np.empty((height, width, 4), np.uint8), "depth": np.empty((height, width), F),
           "prequant": np.empty((height, width, 4), F), "draw_id": np.empty((height, width), np.int32),
           "texel": np.empty((height, width), np.int32)}
    rc = ref_lib().rlt_render(width, height, tile[0], tile[1], arr, len(draws),
                              *[out[k].ctypes.data for k in ("color", "depth", "prequant", "draw_id", "texel")])
    assert rc >= 0
    out["skipped"] = int(rc)
    return out


def ref_sample(tex, uv):
    uv = np.ascontiguousarray(np.asarray(uv, F).reshape(-1, 2))
    rgba = np.zeros((uv.shape[0], 4), np.uint8)
    index = np.zeros(uv.shape[0], np.int32)
    assert ref_lib().rlt_sample_nearest(tex.rgba.ctypes.data, tex.rgba.shape[1], tex.rgba.shape[0], uv.shape[0],
                                        uv.ctypes.data, rgba.ctypes.data, index.ctypes.data) == 0
    return rgba, index


def covered(planes):
    return planes["depth"][::-1] < helpers.FLT_MAX   # canvas rows


# ---- textures ---------------------------------------------------------------------------------------------
# Texel (x, y) = (R0 + RS x, G0 + GS y, 100): pairwise distinct, and dark enough that the lit colour
# s * texel / 255 (s <= 0.15 + 1 + 0.5) never reaches the clamp -- so the ratio of a pixel's pre-truncation
# red and green to its blue gives its texel back (texel_of_prequant): a wrong texel is a wrong index, not a
# near miss in a byte.
def coded_texture(w, h, r0=10, rs=1, g0=10, gs=1):
    t = np.zeros((h, w, 4), np.uint8)
    t[..., 0] = r0 + rs * np.arange(w)[None, :]
    t[..., 1] = g0 + gs * np.arange(h)[:, None]
    t[..., 2] = 100
    t[..., 3] = (np.arange(w)[None, :] * 7 + np.arange(h)[:, None] * 13) % 256   # (alpha is never read)
    assert t[..., :2].max() <= 120
    tex = Tex(t)
    tex.code = (r0, rs, g0, gs)
    return tex


def texel_of_prequant(tex, pq):
    """The texel index (y * w + x) each pixel's pre-truncation floats pq [..., 4] were shaded from."""
    r0, rs, g0, gs = tex.code
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.rint((pq[..., 0].astype(np.float64) / pq[..., 2] * 100.0 - r0) / rs)
        y = np.rint((pq[..., 1].astype(np.float64) / pq[..., 2] * 100.0 - g0) / gs)
    ok = np.isfinite(x) & np.isfinite(y)
    return np.where(ok, np.where(ok, y, 0).astype(np.int64) * tex.rgba.shape[1] + np.where(ok, x, 0).astype(np.int64), -1)


TEX_A = coded_texture(64, 48)
TEX_B = coded_texture(2, 3, 20, 40, 20, 30)
TEX_1 = coded_texture(1, 1, 60, 1, 90, 1)


# ---- the scenes -------------------------------------------------------------------------------------------
def _draw(mesh, model, view, proj, cam_pos, tex, color=COLOR, shading=TEXTURED):
    from shs_gpu import scene
    d = scene.make_draw(mesh, shading, model, view, proj, scene.glm_normalize(LIGHT), cam_pos, color)
    d.albedo_tex = tex
    return d


def scene_a(tex=TEX_A, cam_pos=CAM, yaw=0.0, pitch=0.0):
    """Scene A: the monkey of test_legacy_shaders_ref.monkey_draw with its own UVs."""
    from shs_gpu import scene
    view, proj = scene.camera(cam_pos, yaw, pitch)
    model = scene.model_trs((0.0, 0.0, 10.0), -30.0, (4.0, 4.0, 4.0))
    return [_draw(scene.monkey(), model, view, proj, cam_pos, tex)]


def _quad(x0, x1, z0, z1, uv0=-0.25, uv1=1.25):
    """A ground quad (y = 0, normal up) of two triangles, front-facing from above; u runs with x, v with z."""
    p = [(x0, 0.0, z0), (x0, 0.0, z1), (x1, 0.0, z1), (x1, 0.0, z0)]
    t = [(uv0, uv0), (uv0, uv1), (uv1, uv1), (uv1, uv0)]
    tri = [(0, 1, 2), (0, 2, 3)]
    pos = np.array([[c for i in tr for c in p[i]] for tr in tri], F)
    uvs = np.array([[c for i in tr for c in t[i]] for tr in tri], F)
    nrm = np.tile(np.array([0.0, 1.0, 0.0], F), (2, 3))
    return SoupMesh(pos, nrm, uvs)


QUAD = _quad(-6.0, 6.0, 1.5, 60.0)
CAM_B = (0.0, 1.2, 0.0)


def scene_b(cam_pos=CAM_B, yaw=0.0, pitch=-4.0):
    """Scene B: the ground quad seen at a grazing angle from 1.2 above it -- w runs from ~1.5 to ~60 across it --
    drawn twice side by side: UVs -0.25 .. 1.25 over a 2x3 and over a 1x1 texture."""
    from shs_gpu import scene
    view, proj = scene.camera(cam_pos, yaw, pitch)
    left = scene.model_trs((-6.5, 0.0, 0.0), 0.0, (1.0, 1.0, 1.0))
    right = scene.model_trs((6.5, 0.0, 0.0), 0.0, (1.0, 1.0, 1.0))
    return [_draw(QUAD, left, view, proj, cam_pos, TEX_B), _draw(QUAD, right, view, proj, cam_pos, TEX_1)]


# One corner behind the camera (w < 0): its screen position is mirrored through the centre, and this winding
# keeps area > 0 (texture_mapping.cpp:245-246), so the triangle is rastered -- and the pixels whose invw_sum
# is <= 0 are skipped (:257).
TRI_C = SoupMesh(np.array([[2.5, -0.75, 5.0, -3.75, -1.5, 5.0, -2.5, -1.0, -1.25]], F),
                 np.tile(np.array([0.0, 0.0, -1.0], F), (1, 3)),
                 np.array([[0.0, 0.0, 0.5, 1.0, 1.0, 0.0]], F))
CAM_C = (0.0, 1.0, 0.0)


def scene_c():
    from shs_gpu import scene
    view, proj = scene.camera(CAM_C, 0.0, 0.0)
    model = scene.model_trs((0.0, 0.0, 0.0), 0.0, (1.0, 1.0, 1.0))
    return [_draw(TRI_C, model, view, proj, CAM_C, TEX_A)]


SCENES = {"A": scene_a, "B": scene_b, "C": scene_c}


@functools.lru_cache(maxsize=None)
def scene_frame(name):
    draws = SCENES[name]()
    return draws, ref_render(W, H, draws)


def corner_w(draw):
    """The clip-space w of every corner of the draw's mesh."""
    from shs_gpu import scene
    p = draw.mesh.positions.reshape(-1, 3)
    return np.array([scene.glm_m4v4(draw.mvp, (*c, 1.0))[3] for c in p], F)


# ---- the sampler's edge sets ------------------------------------------------------------------------------
NAN = float("nan")


def sampler_sets():
    """(texture, uv [n, 2], the expected texel indices or None) per case."""
    sets = []
    sets.append((TEX_1, [(0.0, 0.0), (0.7, 0.2), (-3.0, 9.0), (NAN, NAN), (1.0, 1.0)], [0, 0, 0, 0, 0]))
    # u (w - 1) exactly on .5: std::lround rounds halves away from zero (to-even would give 0, 2, 2)
    for w, want in ((2, 1), (4, 2), (6, 3)):
        t = coded_texture(w, 1, 10, 10, 10, 1)
        sets.append((t, [(0.5, 0.0)], [want]))
    t = coded_texture(5, 4, 10, 10, 10, 10)
    sets.append((t, [(0.125, 0.0), (0.375, 0.5), (0.625, 1.0 / 6.0), (0.875, 0.5)], [1, 2 * 5 + 2, 1 * 5 + 3, 2 * 5 + 4]))
    sets.append((t, [(-0.25, -1e-9), (1.25, 1.0 + 1e-6), (-np.inf, np.inf), (2.0, -2.0)], [0, 3 * 5 + 4, 3 * 5 + 0, 0 * 5 + 4]))
    # a NaN coordinate stays NaN through saturate; lroundf(NaN) on x86-64 glibc is LONG_MIN, whose (int) is 0
    sets.append((t, [(NAN, 0.5), (0.5, NAN), (NAN, NAN)], [2 * 5 + 0, 0 * 5 + 2, 0]))
    rng = np.random.default_rng(5)
    sets.append((TEX_A, rng.uniform(-0.5, 1.5, (400, 2)).astype(F), None))
    sets.append((TEX_B, rng.uniform(-0.5, 1.5, (200, 2)).astype(F), None))
    return sets


def np_sample_index(tex, uv):
    """sample_nearest's texel index in float32 numpy (NaN coordinates: column / row 0)."""
    h, w = tex.rgba.shape[:2]
    uv = np.asarray(uv, F).reshape(-1, 2)

    def coord(c, n):
        s = np.where(c < 0, F(0), np.where(c > 1, F(1), c)).astype(F)
        x = (s * F(n - 1)).astype(F)
        t = np.trunc(x)
        with np.errstate(invalid="ignore"):
            i = np.where(np.isnan(x), 0, t + ((x - t) >= F(0.5)))
        return np.clip(np.where(np.isnan(i), 0, i).astype(np.int64), 0, n - 1)

    return coord(uv[:, 1], h) * w + coord(uv[:, 0], w)


# ---- float32 numpy restatement of the pipeline (independent of the C text) --------------------------------
def _m4(m, p):
    m = np.asarray(m, F)
    x, y, z = F(p[0]), F(p[1]), F(p[2])
    return [F(F(m[r] * x + m[4 + r] * y) + F(m[8 + r] * z + m[12 + r] * F(1))) for r in range(4)]


def _norm(v):
    d = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    inv = F(1.0) / np.sqrt(d)
    return [v[0] * inv, v[1] * inv, v[2] * inv]


def np_render(width, height, draws, tile=(80, 80)):
    """Every pixel against every triangle, whole-frame float32 arrays, in the reference's operation order.
    The tile clamp is applied per tile job.  -> depth (screen rows), texel and prequant (canvas rows)."""
    depth = np.full((height, width), helpers.FLT_MAX, F)
    texel = np.full((height, width), -1, np.int64)
    pq = np.zeros((height, width, 4), F)
    ys, xs = np.mgrid[0:height, 0:width]
    Px, Py = (xs + 0.5).astype(F), (ys + 0.5).astype(F)
    tjx, tjy = xs // tile[0], ys // tile[1]
    tminx, tminy = (tjx * tile[0]).astype(F), (tjy * tile[1]).astype(F)
    tmaxx = (np.minimum((tjx + 1) * tile[0], width) - 1).astype(F)
    tmaxy = (np.minimum((tjy + 1) * tile[1], height) - 1).astype(F)
    gmin = lambda a, b: np.where(b < a, b, a)
    gmax = lambda a, b: np.where(a < b, b, a)
    for d in draws:
        model = np.asarray(d.model, F)
        inv = np.linalg.inv(model.reshape(4, 4).T.astype(np.float64))   # (the scenes' models: exact in float32)
        nmat = inv.T[:3, :3].astype(F)
        uvs = getattr(d.mesh, "uvs", None)
        for ti in range(d.mesh.positions.shape[0]):
            P3 = d.mesh.positions[ti].reshape(3, 3)
            N3 = d.mesh.normals[ti].reshape(3, 3)
            T3 = np.zeros((3, 2), F) if uvs is None else uvs[ti].reshape(3, 2)
            clip = [_m4(d.mvp, p) for p in P3]
            wp = [_m4(d.model, p)[:3] for p in P3]
            nr = [_norm([F(F(nmat[r, 0] * n[0] + nmat[r, 1] * n[1]) + nmat[r, 2] * n[2]) for r in range(3)]) for n in N3]
            sx = [F(F(F(c[0] / c[3]) + F(1)) * F(0.5)) * F(width - 1) for c in clip]
            sy = [F(F(F(1) - F(c[1] / c[3])) * F(0.5)) * F(height - 1) for c in clip]
            iw = [F(1) / c[3] for c in clip]
            q = [F(F(c[2] * i) * i) for c, i in zip(clip, iw)]
            area = F(F(sx[1] - sx[0]) * F(sy[2] - sy[0])) - F(F(sy[1] - sy[0]) * F(sx[2] - sx[0]))
            if not area > 0:
                continue
            bminx, bminy, bmaxx, bmaxy = tmaxx, tmaxy, tminx, tminy
            for k in range(3):
                bminx = gmax(tminx, gmin(bminx, sx[k])); bminy = gmax(tminy, gmin(bminy, sy[k]))
                bmaxx = gmin(tmaxx, gmax(bmaxx, sx[k])); bmaxy = gmin(tmaxy, gmax(bmaxy, sy[k]))
            visit = ~((bminx > bmaxx) | (bminy > bmaxy)) & (xs >= bminx.astype(np.int64)) & (xs <= bmaxx.astype(np.int64)) & \
                (ys >= bminy.astype(np.int64)) & (ys <= bmaxy.astype(np.int64))
            v0x, v0y, v1x, v1y = F(sx[1] - sx[0]), F(sy[1] - sy[0]), F(sx[2] - sx[0]), F(sy[2] - sy[0])
            v2x, v2y = Px - sx[0], Py - sy[0]
            d00, d01, d11 = F(v0x * v0x) + F(v0y * v0y), F(v0x * v1x) + F(v0y * v1y), F(v1x * v1x) + F(v1y * v1y)
            d20, d21 = v2x * v0x + v2y * v0y, v2x * v1x + v2y * v1y
            den = F(d00 * d11) - F(d01 * d01)
            if abs(float(den)) < 1e-5:
                continue
            bv, bw = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
            bu = (F(1) - bv) - bw
            s = (bu * iw[0] + bv * iw[1]) + bw * iw[2]
            with np.errstate(divide="ignore", invalid="ignore"):
                z = ((bu * q[0] + bv * q[1]) + bw * q[2]) / s
                win = visit & ~((bu < 0) | (bv < 0) | (bw < 0)) & ~(s <= 0) & (z < depth)
                depth = np.where(win, z, depth)
                if not win.any():
                    continue
                nsum = [(bu * nr[0][c] + bv * nr[1][c]) + bw * nr[2][c] for c in range(3)]
                wpos = [((bu * F(wp[0][c] * iw[0]) + bv * F(wp[1][c] * iw[1])) + bw * F(wp[2][c] * iw[2])) / s for c in range(3)]
                uv = [((bu * F(T3[0][c] * iw[0]) + bv * F(T3[1][c] * iw[1])) + bw * F(T3[2][c] * iw[2])) / s for c in range(2)]
                n1 = _norm(_norm(nsum))
                L = _norm([F(-d.light_dir[0]), F(-d.light_dir[1]), F(-d.light_dir[2])])
                V = _norm([F(d.camera_pos[c]) - wpos[c] for c in range(3)])
                diff = gmax((n1[0] * L[0] + n1[1] * L[1]) + n1[2] * L[2], F(0))
                Hh = _norm([L[c] + V[c] for c in range(3)])
                spec = np.power(gmax((n1[0] * Hh[0] + n1[1] * Hh[1]) + n1[2] * Hh[2], F(0)), F(64.0)).astype(F)
                lit = (F(0.15) + diff) + F(0.5) * spec
            tex = texture_of(d)
            if tex is not None:
                idx = np_sample_index(tex, np.stack([uv[0], uv[1]], -1).reshape(-1, 2)).reshape(height, width)
                base = tex.rgba.reshape(-1, 4)[idx][..., :3].astype(F) / F(255.0)
            else:
                idx = np.full((height, width), -1, np.int64)
                base = np.broadcast_to(np.asarray(d.color[:3], F) / F(255.0), (height, width, 3))
            pre = np.stack([gmin(gmax(lit * base[..., c], F(0)), F(1)) * F(255) for c in range(3)] + [np.ones_like(lit)], -1)
            texel = np.where(win, idx, texel)
            pq = np.where(win[..., None], pre.astype(F), pq)
    return {"depth": depth, "texel": texel[::-1], "prequant": pq[::-1]}


# ---- the tests --------------------------------------------------------------------------------------------
def test_equal_w_frame_relates_to_the_oracles_blinn_phong(oracle_mod):
    from shs_gpu import scene
    # x, y scaled into NDC, z into (0, 1), last row (0, 0, 0, 1): w = 1 at every corner
    mvp = np.zeros(16, F)
    mvp[0], mvp[5], mvp[10], mvp[15] = 0.6, 0.7, 0.1, 1.0
    mvp[12], mvp[13], mvp[14] = 0.05, -0.1, 0.5
    model = scene.model_trs((0.0, 0.0, 10.0), -30.0, (4.0, 4.0, 4.0))
    mesh = scene.monkey()
    d9 = scene.Draw(mesh, TEXTURED, mvp, model, scene.glm_normalize(LIGHT), np.asarray(CAM, F), COLOR)
    d3 = copy.copy(d9)
    d3.shading = BLINN
    assert (corner_w(d9) == 1.0).all()
    ref = ref_render(W, H, [d9])
    ora_c, ora_d, _ = oracle_mod.render_legacy(W, H, [d3], prequant=True)
    cov = ora_d < helpers.FLT_MAX
    assert cov.sum() > 2000 and ref["skipped"] == 0
    assert np.array_equal(ref["depth"] < helpers.FLT_MAX, cov), "coverage differs"
    # z = z_affine / s with s = (u + v) + w, where u = (1 - v) - w: at most two roundings from 1
    rel = np.abs(ref["depth"][cov].astype(np.float64) - ora_d[cov]) / np.abs(ora_d[cov])
    assert rel.max() <= 4 * 2.0 ** -24, rel.max()
    assert np.array_equal(ref["color"], ora_c), "texture-less colour bytes differ from the oracle's Blinn-Phong"
    assert (ref["texel"] == -1).all()


def test_sampler_equals_numpy_and_known_answers():
    for tex, uv, want in sampler_sets():
        rgba, index = ref_sample(tex, uv)
        assert np.array_equal(index, np_sample_index(tex, uv))
        if want is not None:
            assert index.tolist() == want, (index.tolist(), want)
        assert np.array_equal(rgba[:, :3], tex.rgba.reshape(-1, 4)[index][:, :3]) and (rgba[:, 3] == 255).all()


@functools.lru_cache(maxsize=None)
def two_triangle_draws():
    """The numpy restatement's scene: Scene B's left quad, once textured, once without a texture (at another
    place), once without UVs."""
    b = scene_b()
    plain = copy.copy(b[1])
    plain.albedo_tex = 0
    no_uv = copy.copy(b[0])
    no_uv.mesh = SoupMesh(QUAD.positions, QUAD.normals, None)
    return {"textured": [b[0]], "no_texture": [plain], "no_uvs": [no_uv]}


def test_raster_equals_numpy_restatement():
    for name, draws in two_triangle_draws().items():
        ref = ref_render(W, H, draws)
        mine = np_render(W, H, draws)
        assert covered(ref).sum() > 300, name
        helpers.assert_depth_bitexact(mine["depth"], ref["depth"])
        assert np.array_equal(mine["texel"], ref["texel"]), name
        dp = np.abs(mine["prequant"][..., :3] - ref["prequant"][..., :3])
        assert dp.max() <= helpers.TOL * 255.0, (name, dp.max())
        if name == "no_texture":
            assert (ref["texel"] == -1).all()
        if name == "no_uvs":   # vec2(0) per corner: texel (0, 0) everywhere
            assert (ref["texel"][covered(ref)] == 0).all()
        if name == "textured":
            assert len(np.unique(ref["texel"][covered(ref)])) == 6   # every texel of the 2x3 texture shows


def test_scenes_cover_what_the_gpu_tests_need():
    a = scene_frame("A")[1]
    assert covered(a).sum() > 500 and a["skipped"] == 0
    assert len(np.unique(a["texel"][covered(a)])) > 200          # hundreds of the 3072 texels show
    draws, b = scene_frame("B")
    w = np.concatenate([corner_w(d) for d in draws])
    assert w.min() > 0 and w.max() / w.min() >= 20.0
    for k in range(2):
        assert (b["draw_id"] == k).sum() > 300
    assert b["skipped"] == 0
    assert set(np.unique(b["texel"][b["draw_id"] == 0])) == set(range(6)) and (b["texel"][b["draw_id"] == 1] == 0).all()
    draws, c = scene_frame("C")
    assert (corner_w(draws[0]) < 0).sum() == 1
    assert covered(c).sum() > 300 and c["skipped"] > 300          # kept and skipped pixels, a few hundred each
    # (perspective: the far texel rows of the 2x3 texture take a few pixels each, the near one thousands)
    count = np.bincount(b["texel"][b["draw_id"] == 0], minlength=6)
    assert (count > 5).all() and count.max() > 50 * count.min()
