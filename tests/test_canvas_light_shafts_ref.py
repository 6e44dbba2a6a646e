"""tests/canvas_light_shafts_ref (ref_canvas_light_shafts.c), the C restatement of light_shafts_pass
(hello-render-target/hello_pbr_light_shafts.cpp:1390-1707) -- the reference of tests/test_canvas_light_shafts.py --
pinned on the CPU:

  * against a second restatement in float32 numpy, written from the same cited lines, bit for bit in everything the
    pass derives before a transcendental: ray_max, view_dir, and per visited step t, wp, uv, z and vis;
  * by known answers: a disabled pass is the identity, one noiseless unjittered step without a map has a closed form,
    a singular inv_view_proj sends every ray along (0, 0, 1), a map of FLT_MAX is no map;
  * against its own variant with the transcendentals in double rounded once to float: the accumulated-step counts of
    the two may differ on at most a quarter of the pixels the GPU test allows (1 in 2,000 marched pixels);
  * with the ABI struct's size against the ctypes mirror, and the parameter sets are checked, on the restatement alone,
    to reach the branches they are there for.

It also holds what fails without the feature and needs no GPU: the new entry points and the struct."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import helpers
import test_canvas_rt_ref as R
from test_canvas_rt_ref import F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_light_shafts_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_light_shafts_ref.so")
_P = ctypes.c_void_p
FLT_MAX = helpers.FLT_MAX

SIZES = ((160, 120), (96, 72))     # 5 x 15 and 3 x 9 tiles of 32 x 8
MAP_SIZES = ((96, 96), (96, 64))
SUN_DIR = R.LIGHT_DIR              # sun -> scene, not normalised

# LightShaftParams over the demo's defaults; each set is there for a branch (test_parameter_sets_reach_their_branches)
PARAM_SETS = {
    "demo": {},
    "thick": dict(steps=24, max_dist=60.0, base_density=2.5, noise_strength=1.0, sigma_s=0.3, sigma_t=0.9),
    "thin": dict(height_falloff=4.0),
    "far_start": dict(steps=16, max_dist=40.0, min_dist=9.0, jitter_amount=0.5),
    "one_step": dict(steps=1, g=-0.5, jitter_amount=0.0, noise_strength=0.0),
}
VARIANTS = {
    "demo_no_shadow": dict(use_shadow=False),
    "demo_no_pcf": dict(shadow_pcf_2x2=False),
    "demo_disabled": dict(enable=False),
}
ALL_SETS = {**PARAM_SETS, **VARIANTS}


class RefDebug(ctypes.Structure):
    _fields_ = [("ray_max", _P), ("view_dir", _P), ("steps", _P), ("visited", _P)]


@functools.lru_cache(maxsize=None)
def ref_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    from shs_gpu import _abi
    L = ctypes.CDLL(REF_LIB)
    L.rls_pass.restype = ctypes.c_int
    L.rls_pass.argtypes = [ctypes.POINTER(_abi.CanvasLightShaftsDescC), _P, _P, _P, _P, _P, ctypes.c_int, ctypes.POINTER(RefDebug)]
    L.rls_sizeof_desc.restype = ctypes.c_size_t
    L.rls_sizeof_desc.argtypes = []
    return L


# ---- the inputs (shared with tests/test_canvas_light_shafts.py) -----------------------------------------------------

def inverse16(m16):
    """The inverse of a column-major float32[16], through float64 (the pass takes the inverse as an input: any will do)."""
    m = np.asarray(m16, np.float64).reshape(4, 4).T
    return np.ascontiguousarray(np.linalg.inv(m).T).reshape(16).astype(F)


@functools.lru_cache(maxsize=None)
def inputs(size=SIZES[0], map_size=MAP_SIZES[0]):
    """test_canvas_rt_ref's camera and light over its demo scene's shadow map; depth from the floor y = 0 where the
    pixel's ray meets it within 45 units (FLT_MAX above the horizon and beyond); src random bytes, alphas too."""
    w, h = size
    view, proj = R.camera(w, h)
    _, light_vp, draws = R.scene_demo()
    shadow = R.ref_shadow(map_size, light_vp, draws)
    inv_vp = inverse16(R._mul(proj, view))
    cam = np.asarray(R.CAM_POS, np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    ndc = np.stack([(xs + 0.5) / w * 2 - 1, 1 - ((h - 1 - ys) + 0.5) / h * 2, np.ones((h, w)), np.ones((h, w))], -1)
    far = ndc @ inv_vp.astype(np.float64).reshape(4, 4)      # row vector times the transposed column-major matrix
    d = far[..., :3] / far[..., 3:] - cam
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(d[..., 1] < 0, -cam[1] / d[..., 1], np.inf)
    hit = cam + d * np.where(np.isfinite(s), s, 0.0)[..., None]
    vm = np.asarray(view, np.float64).reshape(4, 4)          # vm[c][r]
    view_z = hit @ vm[:3, 2] + vm[3, 2]
    depth = np.where(np.isfinite(s) & (s < 45.0), view_z, FLT_MAX).astype(F)
    rng = np.random.default_rng(w * 1000 + h)
    src = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    src[..., 3] = np.where(rng.random((h, w)) < 0.8, 255, src[..., 3])
    return dict(w=w, h=h, cam_pos=R.CAM_POS, inv_vp=inv_vp, light_vp=np.asarray(light_vp, F).reshape(16), sun=SUN_DIR,
                shadow=shadow, depth=np.ascontiguousarray(depth), src=np.ascontiguousarray(src))


def make_desc(inp, params, shadow=True):
    import shs_gpu
    from shs_gpu import _abi
    vals = dict(shs_gpu.Context.LIGHT_SHAFTS_DEFAULTS)
    vals.update(params)
    d = _abi.CanvasLightShaftsDescC()
    d.width, d.height = inp["w"], inp["h"]
    for k in range(3):
        d.cam_pos[k], d.sun_dir_world[k] = float(inp["cam_pos"][k]), float(inp["sun"][k])
    for k in range(16):
        d.inv_view_proj[k], d.light_vp[k] = float(inp["inv_vp"][k]), float(inp["light_vp"][k])
    if shadow is not None and shadow is not False:
        d.shadow_h, d.shadow_w = inp["shadow"].shape if shadow is True else shadow.shape
    for name, ctype in _abi.CanvasLightShaftsDescC._fields_[8:]:
        setattr(d, name, int(vals[name]) if ctype is ctypes.c_int32 else float(vals[name]))
    return d


def ref_pass(inp, params, shadow=True, dbl=False, debug=False):
    """The restatement -> dict(color [h, w, 4], pq [h, w, 4]) and with debug ray_max, view_dir, steps [h, w, n, 8]
    (NaN where a step did not compute the value) and visited.  shadow: True (the inputs' map), an array, or None."""
    w, h = inp["w"], inp["h"]
    d = make_desc(inp, params, shadow)
    sm = inp["shadow"] if shadow is True else shadow
    sm = None if sm is None or sm is False else np.ascontiguousarray(sm, F)
    out = dict(color=np.empty((h, w, 4), np.uint8), pq=np.empty((h, w, 4), F))
    dbg = None
    if debug:
        n = max(1, d.steps)
        out.update(ray_max=np.full((h, w), np.nan, F), view_dir=np.full((h, w, 3), np.nan, F),
                   steps=np.full((h, w, n, 8), np.nan, F), visited=np.zeros((h, w), np.int32))
        dbg = RefDebug(out["ray_max"].ctypes.data, out["view_dir"].ctypes.data, out["steps"].ctypes.data, out["visited"].ctypes.data)
    rc = ref_lib().rls_pass(ctypes.byref(d), inp["src"].ctypes.data, inp["depth"].ctypes.data, None if sm is None else sm.ctypes.data,
                            out["color"].ctypes.data, out["pq"].ctypes.data, 1 if dbl else 0, None if dbg is None else ctypes.byref(dbg))
    assert rc == 0
    return out


@functools.lru_cache(maxsize=None)
def case(name, size=SIZES[0], map_size=MAP_SIZES[0], dbl=False):
    """(inputs, parameters, the restatement's output) of a named set: computed once, shared, read only."""
    inp = inputs(size, map_size)
    out = ref_pass(inp, ALL_SETS[name], dbl=dbl)
    for a in out.values():
        a.setflags(write=False)
    return inp, ALL_SETS[name], out


def marched(pq):
    return pq[..., 3] >= 0


def step_cap(n_marched):
    """The GPU test's cap on pixels whose accumulated-step count may differ: 1 in 2,000 marched pixels (9 of 19,200)."""
    return n_marched // 2000


# ---- what fails without the feature, without a GPU -----------------------------------------------------------------

def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in ("shs_canvas_light_shafts", "shs_rt_device_shadow_map"):
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_ctypes_struct_has_the_headers_size(tmp_path):
    from shs_gpu import _abi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shs_gpu.h"\nint main(void) { printf("%zu %zu %zu %d\\n", '
                   'sizeof(shs_canvas_light_shafts_desc), offsetof(shs_canvas_light_shafts_desc, enable), '
                   'offsetof(shs_canvas_light_shafts_desc, shadow_pcf_2x2), SHS_CANVAS_LIGHT_SHAFTS_MAX_STEPS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C = _abi.CanvasLightShaftsDescC
    assert got == [ctypes.sizeof(C), C.enable.offset, C.shadow_pcf_2x2.offset, _abi.CANVAS_LIGHT_SHAFTS_MAX_STEPS]
    assert ref_lib().rls_sizeof_desc() == ctypes.sizeof(C) == 59 * 4


# ---- the second restatement: float32 numpy, everything before a transcendental ----------------------------------------

def _m4v(m, x, y, z, w):
    """glm mat4 * vec4: (c0 x + c1 y) + (c2 z + c3 w), float32 throughout -> four arrays."""
    return [(m[r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r] * w) for r in range(4)]


def np_geometry(inp, params, shadow):
    """ray_max, the marched mask, view_dir, and for every step k with t < ray_max: t, wp, u, v, z, vis (vis as if the
    density test passed), float32 operation by operation as the cited lines."""
    import shs_gpu
    p = dict(shs_gpu.Context.LIGHT_SHAFTS_DEFAULTS)
    p.update(params)
    w, h = inp["w"], inp["h"]
    one, half, zero = F(1.0), F(0.5), F(0.0)
    depth = inp["depth"]
    max_dist, min_dist = F(p["max_dist"]), F(p["min_dist"])
    with np.errstate(all="ignore"):
        zoff = depth - F(0.25)
        inner = np.where(min_dist < zoff, zoff, min_dist)                   # std::max(min_dist, view_z - 0.25f)
        ray_max = np.where(depth != FLT_MAX, np.where(inner < max_dist, inner, max_dist), max_dist).astype(F)
        march = ~(ray_max <= min_dist)
        ys, xs = np.mgrid[0:h, 0:w]
        fx = (xs.astype(F) + half) / F(w)
        fy = ((h - 1 - ys).astype(F) + half) / F(h)
        ndc_x = fx * F(2.0) - one
        ndc_y = one - fy * F(2.0)
        ivp = inp["inv_vp"].astype(F)
        wf = _m4v(ivp, ndc_x, ndc_y, one, one)
        cam = [F(v) for v in inp["cam_pos"]]
        dx, dy, dz = wf[0] / wf[3] - cam[0], wf[1] / wf[3] - cam[1], wf[2] / wf[3] - cam[2]
        ln = np.sqrt((dx * dx + dy * dy) + dz * dz)
        fwd = (np.abs(wf[3]) < F(1e-8)) | (ln < F(1e-6))
        vd = np.stack([np.where(fwd, zero, dx / ln), np.where(fwd, zero, dy / ln), np.where(fwd, one, dz / ln)], -1).astype(F)
        n = max(1, int(p["steps"]))
        ds = ray_max / F(n)
        seed = (xs.astype(np.uint32) * np.uint32(1973)) ^ (ys.astype(np.uint32) * np.uint32(9277))
        rv = (seed & np.uint32(0xFFFF)).astype(F) / F(65536.0)
        t = min_dist + (rv * ds * F(p["jitter_amount"]))
        lvp = inp["light_vp"].astype(F)
        bias = F(p["shadow_bias"])
        steps = np.full((h, w, n, 8), np.nan, F)
        for k in range(n):
            wp = [cam[c] + vd[..., c] * t for c in range(3)]
            rec = steps[:, :, k]
            rec[..., 0] = t
            for c in range(3):
                rec[..., 1 + c] = wp[c]
            vis = np.ones((h, w), F)
            if p["use_shadow"] and shadow is not None:
                sh, sw = shadow.shape
                clip = _m4v(lvp, wp[0], wp[1], wp[2], one)
                okw = ~(np.abs(clip[3]) < F(1e-6))
                nx, ny, nz = clip[0] / clip[3], clip[1] / clip[3], clip[2] / clip[3]
                rec[..., 6] = np.where(okw, nz, np.nan)
                ok = okw & ~((nz < zero) | (nz > one))
                u = nx * half + half
                v = one - (ny * half + half)
                rec[..., 4] = np.where(ok, u, np.nan)
                rec[..., 5] = np.where(ok, v, np.nan)
                us, vs = np.where(ok, u, zero), np.where(ok, v, zero)      # (keeps the integer conversions defined)
                px, py = us * F(sw - 1), vs * F(sh - 1)

                def cmp(xi, yi):
                    d = shadow[np.clip(yi, 0, sh - 1), np.clip(xi, 0, sw - 1)]
                    return np.where((d == FLT_MAX) | (nz <= d + bias), one, zero)
                if p["shadow_pcf_2x2"]:
                    x0 = np.clip(np.floor(px).astype(np.int64), 0, sw - 1)
                    y0 = np.clip(np.floor(py).astype(np.int64), 0, sh - 1)
                    f = F(0.25) * (((cmp(x0, y0) + cmp(x0 + 1, y0)) + cmp(x0, y0 + 1)) + cmp(x0 + 1, y0 + 1))
                else:
                    inside = ~((u < zero) | (u > one) | (v < zero) | (v > one))
                    tx, ty = np.trunc(px), np.trunc(py)
                    xi = tx.astype(np.int64) + (px - tx >= half)           # lround: halves away from zero (px >= 0)
                    yi = ty.astype(np.int64) + (py - ty >= half)
                    f = np.where(inside, cmp(xi, yi), one)
                vis = np.where(ok, f, one).astype(F)
            rec[..., 7] = vis
            rec[~(t < ray_max)] = np.nan
            t = t + ds
    return ray_max, march, vd, steps


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def _check_geometry(name, size, map_size=MAP_SIZES[0]):
    inp = inputs(size, map_size)
    params = ALL_SETS[name]
    ref = ref_pass(inp, params, debug=True)
    ray_max, march, vd, steps = np_geometry(inp, params, inp["shadow"])
    assert _same_bits(ref["ray_max"], ray_max)
    assert np.array_equal(marched(ref["pq"]), march)
    assert _same_bits(ref["view_dir"][march], vd[march])
    n = steps.shape[2]
    seen = (np.arange(n)[None, None, :] < ref["visited"][..., None]) & march[..., None]
    assert seen.any()
    # a step the loop entered is one the numpy walk has (t < ray_max); what the C step computed has numpy's bits
    assert not np.isnan(steps[seen][:, 0]).any()
    got, want = ref["steps"][seen], steps[seen]
    have = ~np.isnan(got)
    assert have[:, :4].all()
    assert np.array_equal(got[have].view(np.uint32), want[have].view(np.uint32)), \
        f"{name} {size}: {(got[have].view(np.uint32) != want[have].view(np.uint32)).sum()} step values differ"
    return int(have[:, 7].sum())


def test_geometry_equals_numpy_restatement_bitwise():
    for name in ("demo", "thin", "far_start", "demo_no_pcf"):
        assert _check_geometry(name, SIZES[1]) > 0, name
    assert _check_geometry("one_step", SIZES[0]) > 0
    assert _check_geometry("demo", SIZES[1], MAP_SIZES[1]) > 0


# ---- known answers --------------------------------------------------------------------------------------------------

def test_disabled_pass_is_the_identity():
    for size in SIZES:
        inp, _, out = case("demo_disabled", size)
        assert np.array_equal(out["color"], inp["src"])
        assert (inp["src"][..., 3] != 255).any()
        assert np.array_equal(out["pq"], np.broadcast_to(np.array([0, 0, 0, -1], F), out["pq"].shape))


def test_copied_pixels_keep_their_bytes_and_marched_ones_get_alpha_255():
    inp, _, out = case("far_start")
    m = marched(out["pq"])
    assert 0 < m.sum() < m.size
    assert np.array_equal(out["color"][~m], inp["src"][~m])
    assert (out["color"][m][:, 3] == 255).all() and (inp["src"][m][:, 3] != 255).any()


def test_one_noiseless_step_has_the_closed_form():
    """steps = 1, no jitter, no noise, no map: one sample at t = min_dist with vis = 1, in float64 from the restatement's
    own view_dir.  The float32 chain is some twenty operations and three powf within an ulp each, 6e-8 relative apiece:
    under 2e-6 relative on a value of at most 255, so 1e-3 absolute is generous and far under one byte."""
    inp = inputs()
    p = dict(ALL_SETS["one_step"])
    ref = ref_pass(inp, p, shadow=None, debug=True)
    m = marched(ref["pq"])
    assert m.sum() > 1000 and (ref["visited"][m] == 1).all() and (ref["pq"][m][:, 3] == 1).all()
    import shs_gpu
    q = dict(shs_gpu.Context.LIGHT_SHAFTS_DEFAULTS)
    q.update(p)
    vd = ref["view_dir"].astype(np.float64)
    sun = -np.asarray(SUN_DIR, np.float64) / np.linalg.norm(SUN_DIR)
    cos_t = vd @ sun
    g = q["g"]
    phase = (1 - g * g) / np.maximum(1e-4, 1 + g * g - 2 * g * np.clip(cos_t, -1, 1)) ** 1.5
    gate = np.clip((cos_t - 0.1) / 0.9, 0, 1)
    ray_max = ref["ray_max"].astype(np.float64)
    t = q["min_dist"]
    dens = q["base_density"] * np.exp(-np.maximum(0, inp["cam_pos"][1] + vd[..., 1] * t) * q["height_falloff"])
    scatter = q["sigma_s"] * dens * (phase * gate * q["intensity"] + q["ambient_strength"]) * ray_max * (1 - (t / q["max_dist"]) ** 2)
    ls = scatter[..., None] * np.array([0.92, 0.96, 1.0])
    lin = (inp["src"][..., :3] / 255.0) ** np.float64(F(2.2)) + ls
    lin = np.clip(lin / (1 + lin * 0.15), 0, 1)
    want = lin ** (1 / 2.2) * 255
    err = np.abs(ref["pq"][..., :3].astype(np.float64) - want)[m]
    assert err.max() < 1e-3, err.max()
    assert (ls[m] > 1e-4).all()      # the step did add light


def test_singular_inverse_sends_every_ray_along_z():
    inp = dict(inputs(SIZES[1]))
    inv = inp["inv_vp"].copy()
    inv[3::4] = 0.0                  # the last row: world_far.w = 0
    inp["inv_vp"] = inv
    ref = ref_pass(inp, {}, debug=True)
    m = marched(ref["pq"])
    assert m.any() and np.array_equal(ref["view_dir"][m], np.broadcast_to(np.array([0, 0, 1], F), (int(m.sum()), 3)))
    # cam - far point of length under 1e-6: the second fall-back (the matrix maps every pixel onto the camera)
    inv2 = np.zeros(16, F)
    inv2[12:15] = inp["cam_pos"]
    inv2[15] = 1.0
    inp["inv_vp"] = inv2
    ref2 = ref_pass(inp, {}, debug=True)
    assert np.array_equal(ref2["view_dir"][m], ref["view_dir"][m]) and np.array_equal(ref2["color"], ref["color"])


def test_empty_map_is_no_map():
    inp = inputs(SIZES[1])
    empty = np.full((96, 96), FLT_MAX, F)
    for name in ("demo", "demo_no_pcf"):
        a = ref_pass(inp, ALL_SETS[name], shadow=empty)
        b = ref_pass(inp, ALL_SETS[name], shadow=None)
        assert np.array_equal(a["color"], b["color"]) and _same_bits(a["pq"], b["pq"])
        lit = case(name, SIZES[1])[2]
        assert not np.array_equal(lit["color"], b["color"])      # the real map does cast shadows into the fog


# ---- the parameter sets and the double variant ------------------------------------------------------------------------

def test_parameter_sets_reach_their_branches():
    import shs_gpu
    for size in SIZES:
        inp = inputs(size)
        stat = {}
        for name in PARAM_SETS:
            ref = ref_pass(inp, ALL_SETS[name], debug=True)
            m = marched(ref["pq"])
            n = max(1, dict(shs_gpu.Context.LIGHT_SHAFTS_DEFAULTS, **ALL_SETS[name])["steps"])
            stat[name] = dict(m=m, n=n, acc=ref["pq"][..., 3][m], visited=ref["visited"][m], vis=ref["steps"][..., 7][m])
        s = stat["demo"]
        # whole marches, and marches the jittered start ends at t >= ray_max; every step accumulates
        assert s["m"].all() and (s["visited"] == s["n"]).mean() > 0.1 and (s["visited"] < s["n"]).mean() > 0.1
        assert (s["acc"] == s["visited"]).all()
        seen_vis = s["vis"][~np.isnan(s["vis"])]
        assert set(np.unique(seen_vis)) >= {0.0, 0.25, 0.5, 0.75, 1.0}                 # every PCF weight
        s = stat["thick"]
        assert (s["visited"] < s["n"]).mean() > 0.9 and s["visited"].min() >= 2        # ends at Tm < 0.01
        s = stat["thin"]
        assert (s["acc"] == 0).mean() > 0.05 and ((s["acc"] > 0) & (s["acc"] < s["visited"])).mean() > 0.3
        s = stat["far_start"]
        assert 0.25 < 1.0 - s["m"].mean() < 0.75                                        # pixels only copied
        s = stat["one_step"]
        assert (s["visited"] == 1).all()


def test_double_variant_keeps_the_step_counts_within_a_quarter_of_the_cap():
    for size in SIZES:
        for name in ALL_SETS:
            f = case(name, size)[2]["pq"]
            d = case(name, size, dbl=True)[2]["pq"]
            m = marched(f)
            assert np.array_equal(m, marched(d))
            flips = int((f[..., 3][m] != d[..., 3][m]).sum())
            cap = step_cap(int(m.sum()))
            print(f"{name} {size}: {flips} of {int(m.sum())} marched pixels change their step count (cap {cap})")
            assert 4 * flips <= cap, (name, size, flips, cap)
            same = f[..., 3] == d[..., 3]
            err = np.abs(f[..., :3] - d[..., :3])[same]
            assert err.max() <= helpers.TOL * 255.0, (name, size, float(err.max()))
