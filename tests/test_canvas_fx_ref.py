"""tests/canvas_fx_ref (ref_canvas_fx.c), the C restatement of the Canvas-API post passes of hello_multi_pass.cpp,
hello_camera_and_perobject_motion_blur.cpp and hello_glowing_star.cpp -- the reference of tests/test_canvas_fx.py --
pinned on the CPU:

  * by known answers for every pass (fog at and beyond its ends, the outline around one depth step, FXAA on a constant
    image, the additive pass's saturation, the bright pass below its threshold, at 1 and on a NaN, the flare of a black
    canvas, the velocity blur without velocity or samples);
  * by the branches its shared inputs reach: at every size of the GPU test each branch of fog, outline, FXAA and the
    flare's centre is taken by at least one pixel where the size can reach it, so no GPU case passes by missing one;
  * against its own variant with pow / exp in double rounded once to float (what the kernels evaluate): on fog and
    flare, for every parameter set, a byte differs by at most 1 and only where the pre-conversion floats agree within
    helpers.TOL * 255 -- the reference alone stays within the bar the GPU test applies.

It also holds the inputs, the parameter sets and the chains' restatement (the new passes composed with the oracle's
gaussian_blur_pass, DoF step and combined_motion_blur_pass), and what fails without the feature and needs no GPU."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers
from oracle import oracle
from test_canvas_post import _cam

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "canvas_fx_ref")
REF_LIB = os.path.join(REF_DIR, "_build", "libshs_canvas_fx_ref.so")
_P = ctypes.c_void_p
F = np.float32
FLT_MAX = helpers.FLT_MAX

# 1 pixel, one column, one row, one block, one past a block in both axes, odd, even, the demos' canvas
SIZES = ((1, 1), (1, 7), (7, 1), (64, 4), (65, 5), (67, 45), (128, 96), (380, 280))
SWEEP = (67, 45)

FOG_T0, FOG_INTERIOR, FOG_T1 = 1, 2, 3          # 0: copied
OUTLINE_EDGE, OUTLINE_FLAT = 1, 2               # 0: copied
FXAA_LOW, FXAA_A, FXAA_B = 0, 1, 2
FLARE_CENTRE = 1

# the parameter sets of the two passes with a transcendental (over Context.FX_DEFAULTS)
FOG_SETS = {
    "demo": {},
    "power0": dict(fog_power=0.0),
    "power1": dict(fog_power=1.0),
    "power_neg": dict(fog_power=-0.75),
    "end_before_start": dict(fog_start=80.0, fog_end=20.0),
}
FLARE_SETS = {
    "demo": {},
    "one_ghost": dict(ghost_scales=(0.7,)),
    "eight_ghosts": dict(ghost_scales=(0.2, 0.4, 0.55, 0.85, 1.0, 1.25, 1.6, 2.5), intensity=0.3),
    "no_chroma": dict(chroma_shift_px=0.0),
}


@functools.lru_cache(maxsize=None)
def ref_lib():
    subprocess.run(["make", "-s", "-C", REF_DIR], check=True)
    from shs_gpu import _abi
    L = ctypes.CDLL(REF_LIB)
    D = ctypes.POINTER
    I = ctypes.c_int
    for name, args in (("rfx_velocity_blur", [D(_abi.CanvasVelocityBlurDescC), _P, _P, _P]),
                       ("rfx_fog", [D(_abi.CanvasFogDescC), _P, _P, _P, _P, I, _P]),
                       ("rfx_outline", [D(_abi.CanvasOutlineDescC), _P, _P, _P, _P]),
                       ("rfx_fxaa", [D(_abi.CanvasFxaaDescC), _P, _P, _P]),
                       ("rfx_spec_bright", [D(_abi.CanvasSpecBrightDescC), _P, _P]),
                       ("rfx_additive", [I, I, _P, _P, ctypes.c_float, _P]),
                       ("rfx_lens_flare", [D(_abi.CanvasLensFlareDescC), _P, _P, _P, I, _P])):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = args
    L.rfx_sizeof_descs.restype = ctypes.c_size_t
    L.rfx_sizeof_descs.argtypes = [I]
    return L


def _desc(kind, img, params):
    import shs_gpu
    h, w = img.shape[:2]
    return shs_gpu.Context.fx_desc(kind, w, h, params)


def _c8(a):
    a = np.ascontiguousarray(a, np.uint8)
    assert a.ndim == 3 and a.shape[2] == 4
    return a


# ---- the restatement's passes: arrays in, arrays out ---------------------------------------------------------------

def ref_velocity_blur(src, velocity, **params):
    src, velocity = _c8(src), np.ascontiguousarray(velocity, F)
    out = np.empty_like(src)
    ref_lib().rfx_velocity_blur(ctypes.byref(_desc("velocity_blur", src, params)), src.ctypes.data, velocity.ctypes.data,
                                out.ctypes.data)
    return out


def ref_fog(src, depth, dbl=False, **params):
    """-> dict(color, pq [h, w, 4], branch [h, w])"""
    src, depth = _c8(src), np.ascontiguousarray(depth, F)
    h, w = depth.shape
    out = dict(color=np.empty_like(src), pq=np.empty((h, w, 4), F), branch=np.empty((h, w), np.uint8))
    ref_lib().rfx_fog(ctypes.byref(_desc("fog", src, params)), src.ctypes.data, depth.ctypes.data, out["color"].ctypes.data,
                      out["pq"].ctypes.data, 1 if dbl else 0, out["branch"].ctypes.data)
    return out


def ref_outline(src, depth, branch=False, **params):
    src, depth = _c8(src), np.ascontiguousarray(depth, F)
    out, br = np.empty_like(src), np.empty(depth.shape, np.uint8)
    ref_lib().rfx_outline(ctypes.byref(_desc("outline", src, params)), src.ctypes.data, depth.ctypes.data, out.ctypes.data,
                          br.ctypes.data)
    return (out, br) if branch else out


def ref_fxaa(src, branch=False, **params):
    src = _c8(src)
    out, br = np.empty_like(src), np.empty(src.shape[:2], np.uint8)
    ref_lib().rfx_fxaa(ctypes.byref(_desc("fxaa", src, params)), src.ctypes.data, out.ctypes.data, br.ctypes.data)
    return (out, br) if branch else out


def ref_spec_bright(spec, **params):
    spec = np.ascontiguousarray(spec, F)
    out = np.empty(spec.shape + (4,), np.uint8)
    ref_lib().rfx_spec_bright(ctypes.byref(_desc("spec_bright", spec, params)), spec.ctypes.data, out.ctypes.data)
    return out


def ref_additive(base, add, strength=1.0):
    base, add = _c8(base), _c8(add)
    out = np.empty_like(base)
    ref_lib().rfx_additive(base.shape[1], base.shape[0], base.ctypes.data, add.ctypes.data, float(strength), out.ctypes.data)
    return out


def ref_lens_flare(src, dbl=False, **params):
    """-> dict(color, pq, branch)"""
    src = _c8(src)
    h, w = src.shape[:2]
    out = dict(color=np.empty_like(src), pq=np.empty((h, w, 4), F), branch=np.empty((h, w), np.uint8))
    ref_lib().rfx_lens_flare(ctypes.byref(_desc("lens_flare", src, params)), src.ctypes.data, out["color"].ctypes.data,
                             out["pq"].ctypes.data, 1 if dbl else 0, out["branch"].ctypes.data)
    return out


def ref_dof(color, depth, **params):
    import shs_gpu
    p = dict(shs_gpu.Context.FX_DEFAULTS["dof"], **params)
    return oracle.canvas_dof(color, depth, **p)[0]


# ---- the inputs (shared with tests/test_canvas_fx.py) ----------------------------------------------------------------

# W * H <= 7: depths along the linear index -- two flat neighbours before the fog, an empty pixel, the fog's interior,
# a step of 40 (an edge) into full fog
_TINY_DEPTH = np.array([10.0, 10.25, FLT_MAX, 50.0, 90.0, 90.125, 90.25], F)


@functools.lru_cache(maxsize=None)
def inputs(size):
    """src: a flat third, a third of hard stripes and a diagonal, a third of noise, alphas not all 255.  depth: eight
    terraces from 5 to 100 across the diagonal (flat inside, an edge at each riser; before, inside and beyond the
    fog), a nearer box in the middle (a step), a tenth of the pixels and one corner block empty.  velocity: normal,
    sigma 6 px, a fifth zero.  spec: 0 .. 1.2 (below the threshold, through it, past 1) with one NaN and one +inf.
    Read only."""
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    src = np.empty((h, w, 4), np.uint8)
    src[...] = (90, 140, 200, 255)
    mid = (xx >= w // 3) & (xx < 2 * w // 3)
    stripes = np.where(((xx // 3) % 2 == 0)[..., None], np.array([30, 30, 30, 255]), np.array([220, 200, 180, 255]))
    stripes = np.where((xx - w // 3 > yy)[..., None], stripes, np.array([250, 60, 20, 255]))
    src[mid] = stripes[mid].astype(np.uint8)
    noisy = xx >= 2 * w // 3
    noise = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    src[noisy] = noise[noisy]
    src[..., 3] = np.where(rng.random((h, w)) < 0.8, 255, noise[..., 3])
    if w * h <= 7:
        src[..., :3] = noise[..., :3]
        depth = _TINY_DEPTH[:w * h].reshape(h, w).copy()
        if w * h == 1:
            depth[...] = 50.0
    else:
        s = (xx + yy) / max(w + h - 2, 1)
        depth = (5.0 + 95.0 * np.floor(8 * s).clip(0, 7) / 7.0).astype(F)
        box = (abs(xx - w // 2) <= w // 8) & (abs(yy - h // 2) <= max(h // 8, 0))
        depth[box] -= F(6.0)
        depth += rng.uniform(-0.2, 0.2, (h, w)).astype(F)      # many distinct fog factors; under the edge threshold
        depth[rng.random((h, w)) < 0.1] = FLT_MAX
        depth[: max(h // 6, 1), : max(w // 6, 1)] = FLT_MAX
        depth[h // 2, w // 2] = F(42.0)       # the autofocus centre holds a sample
    vel = rng.normal(0.0, 6.0, (h, w, 2)).astype(F)
    vel[rng.random((h, w)) < 0.2] = 0.0
    spec = (rng.random((h, w)) ** 3 * 1.2).astype(F)
    spec[rng.random((h, w)) < 0.5] *= F(0.1)
    if w * h > 7:
        spec[h // 2, w // 3] = np.nan
        spec[h // 3, w // 2] = np.inf
        spec[0, 0] = 1.0
    out = dict(w=w, h=h, src=src, depth=np.ascontiguousarray(depth, F), vel=vel, spec=spec)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bloom_input(size):
    """What the flare reads: the bright pass of the inputs' spec plane after one bloom iteration.  Read only."""
    b = ref_spec_bright(inputs(size)["spec"])
    b = oracle.canvas_gaussian(oracle.canvas_gaussian(b, True), False)
    b.setflags(write=False)
    return b


def camera_pair(size):
    """(curr_view, curr_proj, prev_view, prev_proj) of a camera that moved, for the combined motion blur."""
    w, h = size
    view, proj = _cam((0.0, 6.0, -18.0), (0.0, 2.0, 0.0), w, h)
    pview, pproj = _cam((0.6, 6.2, -17.5), (0.2, 2.0, 0.0), w, h)
    return dict(curr_view=view, curr_proj=proj, prev_view=pview, prev_proj=pproj)


@functools.lru_cache(maxsize=None)
def fog_case(name, size, dbl=False):
    inp = inputs(size)
    out = ref_fog(inp["src"], inp["depth"], dbl=dbl, **FOG_SETS[name])
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def flare_case(name, size, dbl=False):
    out = ref_lens_flare(bloom_input(size), dbl=dbl, **FLARE_SETS[name])
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the chains: the order of the demos' main loops ------------------------------------------------------------------

def multi_pass_steps(blur_mode, enable_dof, enable_fxaa):
    """The steps of shs_canvas_multi_pass_frame in order (names of the per-pass parameter dicts)."""
    blur = "velocity_blur" if blur_mode == 0 else "motion_blur"
    dof, fxaa = (["dof"] if enable_dof else []), (["fxaa"] if enable_fxaa else [])
    if blur_mode == 2:      # hello_camera_and_perobject_motion_blur.cpp:1544-1606
        return dof + ["fog", "outline", blur] + fxaa
    return [blur] + dof + ["fog", "outline"] + fxaa      # hello_multi_pass.cpp:1379-1426


def ref_step(step, cur, inp, params, aux=None):
    """One chain step of the restatement on the canvas `cur` -> (canvas, prequant or None)."""
    p = params.get(step) or {}
    if step == "velocity_blur":
        return ref_velocity_blur(cur, inp["vel"], **p), None
    if step == "motion_blur":
        return oracle.canvas_motion_blur(cur, inp["depth"], inp["vel"], **p), None
    if step == "dof":
        return ref_dof(cur, inp["depth"], **p), None
    if step == "fog":
        out = ref_fog(cur, inp["depth"], **p)
        return out["color"], out["pq"]
    if step == "outline":
        return ref_outline(cur, inp["depth"], **p), None
    if step == "fxaa":
        return ref_fxaa(cur, **p), None
    raise KeyError(step)


def ref_multi_pass_frame(inp, blur_mode=0, enable_dof=True, enable_fxaa=True, **params):
    cur = inp["src"]
    for step in multi_pass_steps(blur_mode, enable_dof, enable_fxaa):
        cur, _ = ref_step(step, cur, inp, params)
    return cur


def glow_params(params):
    import shs_gpu
    g = shs_gpu.Context.GLOW_DEFAULTS
    return {k: dict(g.get(k, {}), **(params.get(k) or {})) for k in ("velocity_blur", "dof", "spec_bright", "lens_flare")}


def ref_glow_frame(inp, enable_dof=True, enable_bloom=True, enable_flare=True, bloom_iterations=10, stages=False, **params):
    """hello_glowing_star.cpp:1233-1310 -> the frame, or with stages a dict of every canvas of the chain."""
    p = glow_params(params)
    black = np.zeros_like(inp["src"])
    black[..., 3] = 255
    st = dict(mb=ref_velocity_blur(inp["src"], inp["vel"], **p["velocity_blur"]))
    st["dof"] = ref_dof(st["mb"], inp["depth"], **p["dof"]) if enable_dof else st["mb"]
    if enable_bloom:
        b = ref_spec_bright(inp["spec"], **p["spec_bright"])
        for _ in range(bloom_iterations):
            b = oracle.canvas_gaussian(oracle.canvas_gaussian(b, True), False)
        st["bloom"] = b
    else:
        st["bloom"] = black
    fl = ref_lens_flare(st["bloom"], **p["lens_flare"]) if enable_flare else dict(color=black, pq=None)
    st["flare"], st["flare_pq"] = fl["color"], fl["pq"]
    st["final"] = ref_additive(ref_additive(st["dof"], st["bloom"], 1.0), st["flare"], 1.0)
    return st if stages else st["final"]


# ---- what fails without the feature, without a GPU ------------------------------------------------------------------

ENTRIES = ("shs_canvas_velocity_blur", "shs_canvas_fog", "shs_canvas_outline", "shs_canvas_fxaa", "shs_canvas_spec_bright",
           "shs_canvas_additive", "shs_canvas_lens_flare", "shs_canvas_multi_pass_frame", "shs_canvas_glow_frame")


def test_library_exports_the_entry_points_and_abi_is_unchanged():
    from shs_gpu import _abi
    L = _abi.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert L.shs_abi_version() == 1


def test_ctypes_structs_have_the_headers_sizes(tmp_path):
    from shs_gpu import _abi
    names = ["velocity_blur", "fog", "outline", "fxaa", "spec_bright", "lens_flare", "multi_pass_frame", "glow_frame"]
    mirrors = [_abi.CanvasVelocityBlurDescC, _abi.CanvasFogDescC, _abi.CanvasOutlineDescC, _abi.CanvasFxaaDescC,
               _abi.CanvasSpecBrightDescC, _abi.CanvasLensFlareDescC, _abi.CanvasMultiPassFrameDescC, _abi.CanvasGlowFrameDescC]
    fmt = " ".join(["%zu"] * (len(names) + 4)) + " %d %d"
    args = ", ".join(f"sizeof(shs_canvas_{n}_desc)" for n in names)
    args += (", offsetof(shs_canvas_multi_pass_frame_desc, fog), offsetof(shs_canvas_multi_pass_frame_desc, fxaa), "
             "offsetof(shs_canvas_glow_frame_desc, lens_flare), offsetof(shs_canvas_lens_flare_desc, ghost_scales), "
             "SHS_CANVAS_MAX_OUTLINE_RADIUS, SHS_CANVAS_MAX_FLARE_GHOSTS")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shs_gpu.h"\n'
                   f'int main(void) {{ printf("{fmt}\\n", {args}); return 0; }}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(m) for m in mirrors]
    want += [_abi.CanvasMultiPassFrameDescC.fog.offset, _abi.CanvasMultiPassFrameDescC.fxaa.offset,
             _abi.CanvasGlowFrameDescC.lens_flare.offset, _abi.CanvasLensFlareDescC.ghost_scales.offset,
             _abi.CANVAS_MAX_OUTLINE_RADIUS, _abi.CANVAS_MAX_FLARE_GHOSTS]
    assert got == want
    assert [ref_lib().rfx_sizeof_descs(k) for k in range(8)] == want[:8]


def test_python_descs_carry_the_demos_constants():
    import shs_gpu
    C = shs_gpu.Context
    fog = C.fx_desc("fog", 380, 280)
    assert (list(fog.fog_color), fog.fog_start, fog.fog_end, fog.fog_power) == ([28, 30, 38, 255], 20.0, 80.0, 1.25)
    fl = C.fx_desc("lens_flare", 8, 8)
    assert fl.n_ghosts == 3 and [F(v) for v in fl.ghost_scales[:3]] == [F(0.55), F(0.85), F(1.25)]
    with pytest.raises(TypeError):
        C.fx_desc("outline", 8, 8, dict(radious=1))
    with pytest.raises(ValueError):
        C.fx_desc("lens_flare", 8, 8, dict(ghost_scales=(1.0,) * 9))


# ---- known answers ------------------------------------------------------------------------------------------------

def _img(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)


def test_fog_known_answers():
    src = _img(6, 9)
    empty = np.full((6, 9), FLT_MAX, F)
    out = ref_fog(src, empty)
    assert np.array_equal(out["color"], src) and (out["branch"] == 0).all()
    assert np.array_equal(out["pq"], np.broadcast_to(np.array([0, 0, 0, -1], F), out["pq"].shape))
    near = ref_fog(src, np.full((6, 9), 20.0, F))                   # depth <= start: t = 0, the input's bytes, alpha 255
    assert np.array_equal(near["color"][..., :3], src[..., :3]) and (near["color"][..., 3] == 255).all()
    assert (near["branch"] == FOG_T0).all()
    assert np.array_equal(ref_fog(src, np.full((6, 9), -3.0, F))["color"], near["color"])
    for d in (80.0, 1e30):                                          # depth >= end: the fog colour
        far = ref_fog(src, np.full((6, 9), d, F))
        assert (far["color"] == np.array([28, 30, 38, 255], np.uint8)).all() and (far["branch"] == FOG_T1).all()
    # fog_end < fog_start: the ramp runs towards the camera
    back = ref_fog(src, np.full((6, 9), 10.0, F), fog_start=80.0, fog_end=20.0)
    assert (back["color"] == np.array([28, 30, 38, 255], np.uint8)).all()
    # half way, power 1: t = smoothstep(0.5) = 0.5
    half = ref_fog(src, np.full((6, 9), 50.0, F), fog_power=1.0)
    want = (F(0.5) * src[..., :3].astype(F) + F(0.5) * np.array([28, 30, 38], F)).astype(np.uint8)
    assert np.array_equal(half["color"][..., :3], want) and (half["branch"] == FOG_INTERIOR).all()


def test_outline_known_answers():
    src = _img(8, 12, 1)
    flat = np.full((8, 12), 7.0, F)
    out, br = ref_outline(src, flat, branch=True)
    assert np.array_equal(out[..., :3], src[..., :3]) and (out[..., 3] == 255).all() and (br == OUTLINE_FLAT).all()
    step = flat.copy()
    step[:, 6:] = 9.0                                               # a step of 2 > 0.75 between columns 5 and 6
    out, br = ref_outline(src, step, branch=True)
    edge = np.zeros((8, 12), bool)
    edge[:, 5:7] = True
    assert np.array_equal(br == OUTLINE_EDGE, edge)
    want = (src[..., :3].astype(F) * (F(1.0) - F(1.0) * F(0.15))).astype(np.int32)
    assert np.array_equal(out[..., :3][edge], want[edge]) and np.array_equal(out[..., :3][~edge], src[..., :3][~edge])
    wide = ref_outline(src, step, branch=True, radius=2)[1]
    assert np.array_equal(wide == OUTLINE_EDGE, np.isin(np.arange(12), (4, 5, 6, 7))[None, :].repeat(8, 0))
    assert (ref_outline(src, step, branch=True, radius=0)[1] == OUTLINE_FLAT).all()
    # an empty centre is copied with its alpha; an empty neighbour is skipped, not an edge
    hole = flat.copy()
    hole[3, 4] = FLT_MAX
    out, br = ref_outline(src, hole, branch=True)
    assert br[3, 4] == 0 and np.array_equal(out[3, 4], src[3, 4]) and (np.delete(br.ravel(), 3 * 12 + 4) == OUTLINE_FLAT).all()


def test_fxaa_constant_image_is_unchanged():
    img = np.empty((9, 11, 4), np.uint8)
    img[...] = (17, 130, 240, 99)
    out, br = ref_fxaa(img, branch=True)
    assert np.array_equal(out, img) and (br == FXAA_LOW).all()


def test_additive_saturates():
    a = np.full((3, 5, 4), 200, np.uint8)
    b = np.full((3, 5, 4), 100, np.uint8)
    assert (ref_additive(a, b)[..., :3] == 255).all() and (ref_additive(a, b)[..., 3] == 255).all()
    assert (ref_additive(a, b, 0.5)[..., :3] == 250).all()
    assert (ref_additive(a, b, 0.0)[..., :3] == 200).all()
    assert (ref_additive(a, b, -4.0)[..., :3] == 200).all()          # mul_color clamps at 0
    assert (ref_additive(a, b, 1e30)[..., :3] == 200).all()          # x86's (int) of a float out of range is INT_MIN: 0


def test_bright_pass_known_answers():
    spec = np.array([[0.0, 0.139, 0.1, -5.0, 1.0, np.nan, np.inf, 7.0]], F)
    out = ref_spec_bright(spec)
    assert (out[0, :4, :3] == 0).all() and (out[..., 3] == 255).all()
    assert (out[0, 4] == (255, 255, 255, 255)).all() and (out[0, 6] == (255, 255, 255, 255)).all() and (out[0, 7, :3] == 255).all()
    assert (out[0, 5] == (0, 0, 0, 255)).all()                       # std::max(0.0f, NaN) = 0
    # threshold = 1: the 1e-6 floor of the denominator
    one = ref_spec_bright(np.array([[1.0, 1.0 + 1e-6, 2.0]], F), threshold=1.0, intensity=1.0)
    assert (one[0, 0, :3] == 0).all() and (one[0, 2] == (255, int(F(255.0) * F(0.88)), int(F(255.0) * F(0.45)), 255)).all()


def test_flare_of_a_black_canvas_is_black():
    black = np.zeros((10, 14, 4), np.uint8)
    out = ref_lens_flare(black)
    assert (out["color"] == (0, 0, 0, 255)).all() and (out["pq"][..., :3] == 0).all() and out["branch"][5, 7] == FLARE_CENTRE
    assert out["branch"].sum() == 1


def test_velocity_blur_copies_without_velocity_or_samples():
    src = _img(7, 10, 3)
    vel = np.random.default_rng(4).normal(0, 5, (7, 10, 2)).astype(F)
    assert np.array_equal(ref_velocity_blur(src, np.zeros_like(vel)), src)
    for samples in (1, 0, -2):
        assert np.array_equal(ref_velocity_blur(src, vel, samples=samples), src)
    out = ref_velocity_blur(src, vel)
    assert not np.array_equal(out, src) and (out[np.hypot(vel[..., 0], vel[..., 1]) >= 0.001][:, 3] == 255).all()
    # two samples: both taps have weight 0, the sum's fall-back divides 0 by 1
    two = ref_velocity_blur(src, np.full_like(vel, 3.0), samples=2)
    assert (two == (0, 0, 0, 255)).all()


# ---- the branches the shared inputs reach ----------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shared_inputs_reach_every_branch(size):
    w, h = size
    inp = inputs(size)
    fog = set(np.unique(fog_case("demo", size)["branch"]))
    outline = set(np.unique(ref_outline(inp["src"], inp["depth"], branch=True)[1]))
    fxaa = set(np.unique(ref_fxaa(inp["src"], branch=True)[1]))
    flare = set(np.unique(flare_case("demo", size)["branch"]))
    if w * h == 1:                       # one pixel: one branch each
        assert fog == {FOG_INTERIOR} and outline == {OUTLINE_FLAT} and fxaa == {FXAA_LOW} and flare == {0}
        return
    assert fog == {0, FOG_T0, FOG_INTERIOR, FOG_T1}
    assert outline == {0, OUTLINE_EDGE, OUTLINE_FLAT}
    if w * h > 7:
        assert fxaa == {FXAA_LOW, FXAA_A, FXAA_B}
        spec = inp["spec"]
        assert (spec < 0.139).any() and (spec >= 1.0).any() and np.isnan(spec).any()
        assert ((spec > 0.139) & (spec < 1.0)).any()
        assert (bloom_input(size)[..., :3] > 0).any() and (flare_case("demo", size)["color"][..., :3] > 0).any()
    else:                                # a line of seven noise pixels: the contrast gate opens, either blend may win
        assert fxaa & {FXAA_A, FXAA_B}
    assert (FLARE_CENTRE in flare) == (w % 2 == 0 and h % 2 == 0)
    # the blur has pixels it copies and pixels it blurs
    vlen = np.hypot(inp["vel"][..., 0], inp["vel"][..., 1])
    assert (vlen < 0.001).any() and (vlen > 1.0).any()


# ---- float libm against double-then-round ---------------------------------------------------------------------------

def _variant_check(f, d, label):
    assert np.array_equal(f["branch"] == 0, d["branch"] == 0)
    n = helpers.assert_color_parity(f["color"], d["color"], f["pq"], d["pq"])
    diff = f["color"] != d["color"]
    if n:
        assert np.abs(f["color"].astype(np.int16) - d["color"].astype(np.int16)).max() <= 1
        gap = np.abs(f["pq"][..., :3] - d["pq"][..., :3])[diff[..., :3]]
        assert (gap <= helpers.TOL * 255.0).all()
    worst = float(np.abs(f["pq"][..., :3].astype(np.float64) - d["pq"][..., :3].astype(np.float64)).max())
    print(f"{label}: {n} bytes differ between the float and the double variant, largest float difference {worst:.3g}")
    assert worst <= helpers.TOL * 255.0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float_variant_stays_within_the_bar_of_the_double_variant(size):
    for name in FOG_SETS:
        _variant_check(fog_case(name, size), fog_case(name, size, dbl=True), f"fog {name} {size}")
    for name in FLARE_SETS:
        _variant_check(flare_case(name, size), flare_case(name, size, dbl=True), f"flare {name} {size}")


def test_chain_restatement_is_the_composition_it_says():
    """The frame restatements against the passes called by hand in the demos' order, at one size."""
    size = SWEEP
    inp = inputs(size)
    cam = camera_pair(size)
    a = ref_velocity_blur(inp["src"], inp["vel"])
    a = ref_dof(a, inp["depth"])
    a = ref_fog(a, inp["depth"])["color"]
    a = ref_fxaa(ref_outline(a, inp["depth"]))
    assert np.array_equal(ref_multi_pass_frame(inp), a)
    b = ref_fog(ref_dof(inp["src"], inp["depth"]), inp["depth"])["color"]
    b = oracle.canvas_motion_blur(ref_outline(b, inp["depth"]), inp["depth"], inp["vel"], **cam)
    assert np.array_equal(ref_multi_pass_frame(inp, blur_mode=2, enable_fxaa=False, motion_blur=cam), b)
    assert multi_pass_steps(1, False, True) == ["motion_blur", "fog", "outline", "fxaa"]
    st = ref_glow_frame(inp, bloom_iterations=2, stages=True)
    assert (st["bloom"][..., :3] > 0).any() and (st["flare"][..., :3] > 0).any()
    assert not np.array_equal(st["final"], st["dof"])
    off = ref_glow_frame(inp, enable_bloom=False, enable_flare=False, stages=True)
    assert np.array_equal(off["final"][..., :3], off["dof"][..., :3]) and (off["final"][..., 3] == 255).all()
