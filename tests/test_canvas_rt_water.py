"""hello_water.cpp's camera passes on the GPU (shs_rt_render_water, shs_rt_frame::shading 5: the atmosphere and the water fragment
shaders chosen per draw, the planar reflection held in the context) against tests/canvas_rt_water_ref
(test_canvas_rt_water_ref.py holds the wrapper, the scenes, what pins the reference on the CPU and the witnesses that show
a wrong normal or texel could not hide under the bar).

Per frame, on every pixel of every plane, none excused (test_canvas_rt_skybox_ibl.compare_planes): the shading sub-triangle,
the view-z depth, the velocity and the shadow factor (the prequant plane's fourth float) equal bit for bit; the colour
floats before the rounding to the byte within helpers.TOL * 255 (a NaN where the reference has a NaN); colour bytes equal
but for a byte off by one where those floats agree within that bound.  PASS0 is the hard demo's and is compared as there."""
import ctypes
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_rt_pbr_ref as P
import test_canvas_rt_ref as R
import test_canvas_rt_sky as TK
import test_canvas_rt_sky_ref as K
import test_canvas_rt_skybox_ibl as TI
import test_canvas_rt_skybox_ibl_ref as I
import test_canvas_rt_water_ref as WR
from test_canvas_rt_ref import F, H, SM, W

pytestmark = pytest.mark.gpu
BAR = helpers.TOL * 255.0
compare_planes = TI.compare_planes
_bits = P.canonical_bits


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def surfaces(flags):
    import shs_gpu
    return [shs_gpu.RtWaterDraw(bool(f)) for f in flags]


def render_scene(c, s):
    """PASS0 if the frame reads the map, the host reflection, PASS1 -> the device's planes"""
    if s.frame.use_shadow:
        c.rt_render_shadow(s.sm, s.light_vp, s.draws, ref_tile=s.tile)
    c.rt_set_reflection(s.reflection if s.water.reflection else None)
    c.rt_render_water(s.frame, s.draws, surfaces(s.surface), s.water)
    return TK._planes(c)


@pytest.mark.parametrize("name", WR.SCENE_NAMES)
def test_scene(ctx, name):
    """Every scene of test_canvas_rt_water_ref.scene (its test_scenes_show_their_edges shows what each one reaches): a host
    reflection of distinct texels at another size than the frame, no reflection, lookups that leave the rndc square or fail
    the |w| test, with and without the map and the PCF under a light box smaller than the water, the water first, absent
    and twice, NaN corners and NaN normals, the times of w = 1, w = 0 and 1e4, a 1 x 1 reflection, a frame one pixel high
    and tile jobs that cut the frame unevenly."""
    s, ref = WR.scene(name), WR.scene_ref(name)
    got = render_scene(ctx, s)
    if s.frame.use_shadow:
        bad = np.argwhere(_bits(ctx.rt_resolve_shadow()) != _bits(ref["shadow_map"]))
        assert bad.size == 0, f"{len(bad)} shadow-map texels differ, first {bad[:4].tolist()}"
    compare_planes(got, ref, name)
    assert ctx.rt_stats() == ref["counters"]


def test_water_samples_equal_the_restatement_bitwise(ctx):
    """shs_rt_water_samples, the device function the raster calls, on the CPU test's seeded points and times: N and foam bit
    for bit."""
    pts = WR.seeded_points()
    for t in WR.sample_times():
        gn, gf = ctx.rt_water_samples(pts, t)
        rn, rf = WR.ref_water_samples(pts, t)
        bad = np.argwhere((_bits(gn) != _bits(rn)).any(-1) | (_bits(gf) != _bits(rf)))
        assert bad.size == 0, f"t = {t}: {len(bad)} of {len(pts)} points differ, first {pts[bad[:3, 0]].tolist()}: {gn[bad[0, 0]]} vs {rn[bad[0, 0]]}"
    n, f = ctx.rt_water_samples(np.zeros((0, 3), F), 1.0)
    assert n.shape == (0, 3) and f.shape == (0,)


def test_the_demos_whole_frame_on_the_device(ctx, oracle_mod):
    """hello_water.cpp's frame at 160 x 120 in its order, enqueued without a resolve in between: the shadow pass, the reflection
    pass from the mirrored camera, shs_rt_keep_reflection, the camera pass with floor, water and objects, and
    shs_canvas_motion_blur with the demo's constants (its combined_motion_blur_pass is the hard demo's routine).  Each stage
    against its restatement; the camera pass over the device's own reflection and the blur over the device's own colour,
    so that a byte the parity rule allows does not travel."""
    import torch
    from shs_gpu import _abi
    _P = ctypes.c_void_p
    d = WR.demo_frame()
    ctx._on_torch_stream()
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    ctx.rt_set_reflection(None)
    ctx.rt_render_shadow(d.sm, d.light_vp, d.main_draws, ref_tile=d.tile)
    ctx.rt_render_water(d.refl_frame, d.refl_draws, surfaces(d.refl_surface), d.refl_water)
    ctx.rt_keep_reflection()
    ctx.rt_render_water(d.main_frame, d.main_draws, surfaces(d.main_surface), d.main_water)
    c_dev, d_dev, v_dev = ctx.rt_device_targets()
    md = _abi.CanvasMotionBlurDescC()
    md.width, md.height = W, H
    for k in range(16):
        md.curr_view[k] = md.prev_view[k] = float(d.view[k])
        md.curr_proj[k] = md.prev_proj[k] = float(d.proj[k])
    md.samples, md.strength, md.w_obj, md.w_cam, md.soft_knee, md.knee_px, md.max_px = 12, 0.85, 1.0, 0.35, 1, 18.0, 22.0
    ctx._check(ctx._lib.shs_canvas_motion_blur(ctx._h, ctypes.byref(md), _P(c_dev), _P(d_dev), _P(v_dev), _P(dst.data_ptr()), ctx.CANVAS_DEVICE))
    ctx.synchronize()
    got = TK._planes(ctx)
    blurred = dst.cpu().numpy()
    ref = WR.demo_frame_ref()
    assert np.array_equal(_bits(ctx.rt_resolve_shadow()), _bits(ref["shadow_map"]))
    # the reflection pass again, alone, against its restatement; its colour is what was kept
    ctx.rt_render_water(d.refl_frame, d.refl_draws, surfaces(d.refl_surface), d.refl_water)
    refl = TK._planes(ctx)
    compare_planes(refl, ref["reflection"], "whole frame, the reflection pass")
    # the camera pass over the device's reflection
    want = WR.ref_render_water(d.main_frame, d.main_draws, d.main_surface, d.main_water, ref["shadow_map"], refl["color"])
    compare_planes(got, want, "whole frame, the camera pass over the kept reflection")
    assert (want["branch"][ref["water_px"]] == WR.REFL_TEXEL).mean() > 0.9
    # the kept canvas equals the reflection pass's resolved colour: the same frame over that colour set from the host
    ctx.rt_set_reflection(refl["color"])
    ctx.rt_render_water(d.main_frame, d.main_draws, surfaces(d.main_surface), d.main_water)
    again = TK._planes(ctx)
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), f"kept against host-set reflection: plane {k} differs"
    # PASS2 over the device's colour
    blur_ref = oracle_mod.canvas_motion_blur(got["color"], got["depth"], got["velocity"], d.view, d.proj, d.view, d.proj)
    bad = np.argwhere((blurred != blur_ref).any(-1))
    assert bad.size == 0, f"{len(bad)} blurred pixels differ, first {bad[:4].tolist()}"
    assert (blurred != got["color"]).any()


def test_kept_reflection_survives_later_passes_and_has_its_own_size(ctx):
    """shs_rt_keep_reflection after a 72 x 48 pass; a 160 x 120 camera pass of another shading and a shadow pass later the water
    still reads those 72 x 48 texels."""
    s = WR.scene("host_reflection")
    ref = WR.scene_ref("host_reflection")
    view, proj = WR.look(WR.GRAZING_POS, WR.GRAZING_TARGET, w=72, h=48)
    small = WR.water_frame(view, s.light_vp, WR.GRAZING_POS, 72, 48, use_shadow=False)
    objs = WR.objects(view, proj)
    ctx.rt_render_water(small, objs, surfaces([False] * 3), dataclasses.replace(s.water, reflection=False))
    ctx.rt_keep_reflection()
    kept = ctx.rt_resolve()[0]
    assert kept.shape == (48, 72, 4)
    hview, _, hdraws = R.scene_demo()
    ctx.rt_render_shadow(s.sm, s.light_vp, s.draws, ref_tile=s.tile)
    ctx.rt_render(R._frame(hview, s.light_vp, use_shadow=False), hdraws)
    ctx.rt_render_water(s.frame, s.draws, surfaces(s.surface), s.water)
    got = TK._planes(ctx)
    want = WR.ref_render_water(s.frame, s.draws, s.surface, s.water, ref["shadow_map"], kept)
    compare_planes(got, want, "a kept 72 x 48 reflection under a 160 x 120 frame")
    ctx.rt_set_reflection(None)


def test_bound_sky_follows_and_is_kept(ctx):
    """A sky bound by shs_rt_set_sky: the background pass follows the shading-5 camera pass as any other, and
    shs_rt_keep_reflection keeps the colour after it."""
    s = WR.scene("no_reflection")
    ref = WR.scene_ref("no_reflection")
    sky = K.analytic_sky(K.elevated(5.0), K.CLAMP, fov_degrees=60.0, **K.camera_of_view(s.frame.view))
    ctx.rt_render_shadow(s.sm, s.light_vp, s.draws, ref_tile=s.tile)
    ctx.rt_set_sky(sky)
    try:
        ctx.rt_render_water(s.frame, s.draws, surfaces(s.surface), s.water)
        got = TK._planes(ctx)
        ctx.rt_keep_reflection()
    finally:
        ctx.rt_set_sky(None)
    want = K.ref_compose(sky, ref)
    compare_planes(got, want, "shading 5 under a bound sky")
    bg = got["tri_id"] < 0
    assert bg.sum() > 500 and (got["color"][bg] != np.array(WR.CLEAR_BG, np.uint8)).any(-1).mean() > 0.99
    # the kept canvas holds the sky: the water of a frame that reads it at identity size shows sky colours where the clear
    # colour would otherwise be read -- compared against the restatement over the device's colour
    h = WR.scene("host_reflection")
    ctx.rt_render_water(h.frame, h.draws, surfaces(h.surface), h.water)
    over = TK._planes(ctx)
    want2 = WR.ref_render_water(h.frame, h.draws, h.surface, h.water, ref["shadow_map"], got["color"])
    compare_planes(over, want2, "the water over a kept frame with its sky")
    ctx.rt_set_reflection(None)


def test_rejections():
    import shs_gpu
    nan, inf = float("nan"), float("inf")
    s, ref = WR.scene("host_reflection"), WR.scene_ref("host_reflection")
    frame, draws, flags, water = s.frame, s.draws, surfaces(s.surface), s.water
    sets = I.knobs_for(draws)
    mats = [P.material(None) for _ in draws]
    with shs_gpu.Context(0) as c:
        def rejected(call, what):
            with pytest.raises(shs_gpu.ShsError) as e:
                call()
            assert e.value.code == -1, what

        def still_right(what):
            c.rt_render_water(frame, draws, flags, water)
            compare_planes(TK._planes(c), ref, f"after the rejection of {what}")

        rejected(lambda: c.rt_keep_reflection(), "shs_rt_keep_reflection before any camera pass")
        rejected(lambda: c.rt_render_water(frame, draws, flags, water), "SHS_RT_USE_SHADOW before any shadow pass")
        c.rt_render_shadow(s.sm, s.light_vp, draws, ref_tile=s.tile)
        rejected(lambda: c.rt_render_water(frame, draws, flags, water), "SHS_RT_WATER_REFLECTION with nothing held")
        c.rt_set_reflection(s.reflection)
        still_right("the reflection flag with nothing held")
        cases = [(f"shading {k}", lambda k=k: c.rt_render_water(dataclasses.replace(frame, shading=k), draws, flags, water)) for k in (0, 1, 2, 3, 4, 6, -1)]
        cases += [("shading 5 through shs_rt_render", lambda: c.rt_render(frame, draws)),
                  ("shading 5 through shs_rt_render_pbr", lambda: c.rt_render_pbr(frame, draws, mats)),
                  ("shading 5 through shs_rt_render_pbr_soft", lambda: c.rt_render_pbr_soft(frame, draws, mats)),
                  ("shading 5 through shs_rt_render_skybox_ibl", lambda: c.rt_render_skybox_ibl(frame, draws, sets)),
                  ("null water_draws", lambda: c.rt_render_water(frame, draws, None, water)),
                  ("null water", lambda: c.rt_render_water(frame, draws, flags, None)),
                  ("unknown draw flags", lambda: c.rt_render_water(frame, draws, [0, 1, 2, 0], water)),
                  ("unknown frame flags", lambda: c.rt_render_water(frame, draws, flags, dataclasses.replace(water, reflection=3))),
                  ("unknown mesh", lambda: c.rt_render_water(frame, [dataclasses.replace(draws[0], mesh=999)] + draws[1:], flags, water)),
                  ("width 0", lambda: c.rt_render_water(dataclasses.replace(frame, width=0), draws, flags, water)),
                  ("a reflection 0 wide", lambda: c._check(c._lib.shs_rt_set_reflection(c._h, s.reflection.ctypes.data, 0, 4)))]
        cases += [(f"time_sec = {bad}", lambda bad=bad: c.rt_render_water(frame, draws, flags, dataclasses.replace(water, time_sec=bad)))
                  for bad in (nan, inf, -inf)]
        cases += [(f"rt_water_samples at {bad}", lambda bad=bad: c.rt_water_samples(np.zeros((2, 3), F), bad)) for bad in (nan, inf)]
        for what, call in cases:
            rejected(call, what)
            still_right(what)
        with pytest.raises(shs_gpu.ShsError):                      # the Python wrapper's own count check
            c.rt_render_water(frame, draws, flags[:-1], water)
        # clearing the canvas takes the flag's ground away again
        c.rt_set_reflection(None)
        rejected(lambda: c.rt_render_water(frame, draws, flags, water), "the reflection flag after the canvas was cleared")
        # no draws and a null table is a frame of the clear colour
        c.rt_render_water(frame, [], None, dataclasses.replace(water, reflection=False))
        assert (c.rt_resolve_ids() == -1).all() and (c.rt_resolve()[0] == np.array(WR.CLEAR_BG, np.uint8)).all()
