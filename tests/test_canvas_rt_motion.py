"""The unclipped camera pass on the GPU (shs_rt_render_motion, shs_rt_frame::shading 6 and 7: the raster of
hello_multi_pass.cpp, hello_camera_and_perobject_motion_blur.cpp and hello_glowing_star.cpp) against
tests/canvas_rt_motion_ref (test_canvas_rt_motion_ref.py holds the wrapper, the scenes, the numpy witness and what pins the
reference on the CPU).

Per frame, on every pixel of every plane, none excused (test_canvas_rt_skybox_ibl.compare_planes): the shading triangle, the
view-z depth and the velocity equal bit for bit (every NaN one NaN); the pre-truncation colour floats within helpers.TOL *
255, a NaN where the reference has a NaN; colour bytes equal but for a byte off by one where those floats agree within that
bound (helpers.assert_color_parity).  The prequant plane's fourth float is bitwise for shading 6 (it is 1).  For shading 7
it is spec01, as the spec plane is: the two are bitwise equal to each other and within helpers.TOL absolute of the
reference's.  Why that bar holds: the operand of pow is bit-identical (no contraction, correctly rounded divide and sqrt);
eight double squarings rounded once and the host powf each lie within one ulp of a value <= 1, and 3.85 times two ulps of 1
is under 5e-7.

The two whole-frame tests enqueue the raster and the demo's post chain without a resolve in between and compare each
stage with its restatement, the chain's (tests/canvas_fx_ref) over the device's own raster output, so that a byte the
parity rule allows does not travel."""
import ctypes
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_fx as FX
import test_canvas_fx_ref as XR
import test_canvas_rt_motion_ref as M
import test_canvas_rt_ref as R
import test_canvas_rt_sky as TK
from test_canvas_rt_motion_ref import H, W
from test_canvas_rt_skybox_ibl import _bits, compare_planes

pytestmark = pytest.mark.gpu
_P = ctypes.c_void_p


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def compare_motion(c, got, ref, shading, label):
    """compare_planes, with the fourth prequant float and the spec plane under shading 7's rule."""
    spec_ref = ref["prequant"][..., 3]
    if shading == 7:
        spec = c.rt_resolve_spec()
        assert np.array_equal(_bits(spec), _bits(got["prequant"][..., 3])), f"{label}: the spec plane is not the prequant plane's fourth float"
        assert np.array_equal(np.isnan(spec), np.isnan(spec_ref)), f"{label}: spec01 is NaN on one side only"
        err = np.nan_to_num(np.abs(spec.astype(np.float64) - spec_ref.astype(np.float64)), nan=0.0)
        print(f"{label}: largest spec01 difference {err.max():.3g} (bar {helpers.TOL:.3g}), {int((_bits(spec) != _bits(spec_ref)).sum())} words not bit-identical")
        assert err.max() <= helpers.TOL, f"{label}: spec01 differs by {err.max()}"
        assert np.array_equal(_bits(ref["spec"]), _bits(spec_ref))
        # the rest under compare_planes, whose fourth-float rule is bitwise: hand it the device's own
        ref = dict(ref, prequant=np.concatenate([ref["prequant"][..., :3], got["prequant"][..., 3:]], -1))
    compare_planes(got, ref, label)


def check_scene(c, name):
    frame, draws = M.scene(name)
    ref = M.scene_ref(name)
    c.rt_render_motion(frame, draws)
    got = TK._planes(c)
    compare_motion(c, got, ref, frame.shading, name)
    assert c.rt_stats() == ref["counters"]
    return got, ref


@pytest.mark.parametrize("name", list(M.SCENES))
def test_scene(ctx, name):
    got, ref = check_scene(ctx, name)
    frame, _ = M.scene(name)
    if frame.shading == 6:
        with pytest.raises(Exception) as e:
            ctx.rt_resolve_spec()
        assert e.value.code == -1
        with pytest.raises(Exception) as e:
            ctx.rt_device_spec()
        assert e.value.code == -1
        assert (got["prequant"][..., 3][got["tri_id"] >= 0] == 1).all()


def test_rejections_leave_a_valid_frame_unchanged():
    import shs_gpu
    frame, draws = M.scene("windings")
    ref = M.scene_ref("windings")
    star, sdraws = M.scene("demo7")
    with shs_gpu.Context(0) as c:
        def rejected(call, what):
            with pytest.raises(shs_gpu.ShsError) as e:
                call()
            assert e.value.code == -1, what

        rejected(c.rt_resolve_spec, "spec before any frame")
        c.rt_render_motion(frame, draws)
        compare_motion(c, TK._planes(c), ref, 6, "before the rejections")
        tex = R.TEX
        cases = [(f"shading {s}", lambda s=s: c.rt_render_motion(dataclasses.replace(frame, shading=s), draws)) for s in (0, 1, 2, 3, 4, 5, 8, -1)]
        cases += [(f"shading {s} through shs_rt_render", lambda s=s: c.rt_render(dataclasses.replace(frame, shading=s), draws)) for s in (6, 7)]
        cases += [("shading 6 through shs_rt_render_pbr", lambda: c.rt_render_pbr(frame, draws, [shs_gpu.RtPbrDraw() for _ in draws])),
                  ("shading 7 through shs_rt_render_skybox_ibl", lambda: c.rt_render_skybox_ibl(dataclasses.replace(frame, shading=7), draws,
                                                                                                [shs_gpu.RtSkyboxIblDraw() for _ in draws])),
                  ("width 0", lambda: c.rt_render_motion(dataclasses.replace(frame, width=0), draws)),
                  ("height -3", lambda: c.rt_render_motion(dataclasses.replace(frame, height=-3), draws)),
                  ("tile 0", lambda: c.rt_render_motion(dataclasses.replace(frame, ref_tile=(0, 80)), draws)),
                  ("SHS_RT_USE_SHADOW", lambda: c.rt_render_motion(dataclasses.replace(frame, use_shadow=True), draws)),
                  ("SHS_RT_PCF", lambda: c.rt_render_motion(dataclasses.replace(frame, pcf=True), draws)),
                  ("albedo_tex", lambda: c.rt_render_motion(frame, [dataclasses.replace(draws[0], albedo_tex=tex)] + draws[1:])),
                  ("unknown mesh", lambda: c.rt_render_motion(frame, [dataclasses.replace(draws[0], mesh=999)] + draws[1:]))]
        cases += [(f"max_velocity_px {v}", lambda v=v: c.rt_render_motion(dataclasses.replace(frame, max_velocity_px=v), draws))
                  for v in (float("nan"), float("inf"), -1.0)]
        for what, call in cases:
            rejected(call, what)
            compare_motion(c, TK._planes(c), ref, 6, f"after the rejection of {what}")
            rejected(c.rt_resolve_spec, f"spec after a shading-6 frame and the rejection of {what}")
        # unknown flag bits, which the Python frame cannot spell
        fc = c._rt_frame_c(frame)
        fc.flags |= 64
        assert c._lib.shs_rt_render_motion(c._h, ctypes.byref(fc), c._rt_draw_array(draws), len(draws)) == -1
        compare_motion(c, TK._planes(c), ref, 6, "after the rejection of unknown flags")
        # a star frame brings the spec plane, a shading-6 frame takes it away again
        c.rt_render_motion(star, sdraws)
        compare_motion(c, TK._planes(c), M.scene_ref("demo7"), 7, "the star after the rejections")
        assert c.rt_device_spec()
        c.rt_render_motion(frame, draws)
        rejected(c.rt_resolve_spec, "spec after a later shading-6 frame")
        rejected(c.rt_device_spec, "device spec after a later shading-6 frame")
        # no draws: the clear
        c.rt_render_motion(star, [])
        assert (c.rt_resolve_ids() == -1).all() and not c.rt_resolve_spec().any()


def test_shading_0_is_undisturbed_by_a_motion_frame(ctx):
    """A shading-0 frame before and after motion frames of both shadings on the same context: bit-identical planes."""
    view, lvp, draws = R.scene_demo()
    ctx.rt_render_shadow(R.SM, lvp, draws)
    ctx.rt_render(R._frame(view, lvp), draws)
    before = TK._planes(ctx)
    stats = ctx.rt_stats()
    for name in ("demo6", "demo7"):
        frame, mdraws = M.scene(name)
        ctx.rt_render_motion(frame, mdraws)
    ctx.rt_render(R._frame(view, lvp), draws)
    after = TK._planes(ctx)
    for k in before:
        assert np.array_equal(after[k].view(np.uint8), before[k].view(np.uint8)), f"plane {k} differs"
    assert ctx.rt_stats() == stats and (before["tri_id"] >= 0).sum() > 3000


def test_sky_background_follows_the_motion_pass(ctx):
    """With a sky bound the background pass colours the pixels the raster left without a fragment, as after every camera
    pass; depth, velocity, ids and the spec plane stay the raster's."""
    import test_canvas_rt_skybox_ibl_ref as I
    frame, draws = M.scene("demo7")
    ref = M.scene_ref("demo7")
    ctx.rt_set_sky(I.demo_sky("analytic"))
    try:
        ctx.rt_render_motion(frame, draws)
        got = TK._planes(ctx)
        spec = ctx.rt_resolve_spec()
    finally:
        ctx.rt_set_sky(None)
    shown = ref["tri_id"] >= 0
    assert np.array_equal(got["tri_id"], ref["tri_id"]) and np.array_equal(_bits(got["depth"]), _bits(ref["depth"]))
    assert np.array_equal(_bits(got["velocity"]), _bits(ref["velocity"]))
    helpers.assert_color_parity(got["color"][shown][None], ref["color"][shown][None], got["prequant"][shown][None], ref["prequant"][shown][None])
    assert (got["color"][~shown] != np.array(frame.clear_color, np.uint8)).any(-1).mean() > 0.99
    assert not spec[~shown].any() and np.abs(spec - ref["spec"]).max() <= helpers.TOL


def _chain_inputs(got, spec=None):
    inp = dict(src=got["color"], depth=got["depth"], vel=got["velocity"])
    if spec is not None:
        inp["spec"] = spec
    return inp


def test_multi_pass_whole_frame_on_the_device(ctx):
    """hello_multi_pass.cpp's frame (blur mode 0) and hello_camera_and_perobject_motion_blur.cpp's order (mode 2) at 160 x
    120: rt_render_motion (shading 6), then shs_canvas_multi_pass_frame over rt_device_targets, nothing resolved in between."""
    import torch
    frame, draws = M.scene("demo6")
    cam = XR.camera_pair((W, H))
    ctx._on_torch_stream()
    ctx.rt_render_motion(frame, draws)
    c_dev, d_dev, v_dev = ctx.rt_device_targets()
    out = {}
    for mode in (0, 2):
        params = dict(motion_blur=cam) if mode else {}
        out[mode] = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        d = ctx.multi_pass_frame_desc(W, H, mode, **params)
        ctx._check(ctx._lib.shs_canvas_multi_pass_frame(ctx._h, ctypes.byref(d), _P(c_dev), _P(d_dev), _P(v_dev), _P(out[mode].data_ptr()),
                                                        ctx.CANVAS_DEVICE))
    ctx.synchronize()
    got = TK._planes(ctx)
    compare_motion(ctx, got, M.scene_ref("demo6"), 6, "whole frame: the raster")
    inp = _chain_inputs(got)
    for mode in (0, 2):
        params = dict(motion_blur=cam) if mode else {}
        cur = inp["src"]
        for step in XR.multi_pass_steps(mode, True, True):
            step_got, step_pq = FX._gpu_step(ctx, step, cur, inp, params)
            if step == "fog":
                FX._check_pq(step_got, step_pq, XR.ref_fog(cur, inp["depth"]), f"whole frame mode {mode}: fog", cur)
            else:
                assert np.array_equal(step_got, XR.ref_step(step, cur, inp, params)[0]), f"whole frame mode {mode}: {step}"
            cur = step_got
        frame_out = out[mode].cpu().numpy()
        assert np.array_equal(frame_out, cur), f"mode {mode}: the chain over the device planes differs from its passes one by one"
        assert not np.array_equal(frame_out, got["color"])
    assert not np.array_equal(out[0].cpu().numpy(), out[2].cpu().numpy())


def test_glow_whole_frame_on_the_device(ctx):
    """hello_glowing_star.cpp's frame at 160 x 120: rt_render_motion (shading 7), then shs_canvas_glow_frame over
    rt_device_targets and rt_device_spec, nothing resolved in between."""
    import shs_gpu
    import torch
    frame, draws = M.scene("demo7")
    ctx._on_torch_stream()
    ctx.rt_render_motion(frame, draws)
    c_dev, d_dev, v_dev = ctx.rt_device_targets()
    s_dev = ctx.rt_device_spec()
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    d = ctx.glow_frame_desc(W, H)
    ctx._check(ctx._lib.shs_canvas_glow_frame(ctx._h, ctypes.byref(d), _P(c_dev), _P(d_dev), _P(v_dev), _P(s_dev), _P(dst.data_ptr()),
                                              ctx.CANVAS_DEVICE))
    ctx.synchronize()
    got = TK._planes(ctx)
    compare_motion(ctx, got, M.scene_ref("demo7"), 7, "whole frame: the star's raster")
    inp = _chain_inputs(got, ctx.rt_resolve_spec())
    p = XR.glow_params({})
    mb = ctx.canvas_velocity_blur(inp["src"], inp["vel"], **p["velocity_blur"])
    assert np.array_equal(mb, XR.ref_velocity_blur(inp["src"], inp["vel"], **p["velocity_blur"]))
    dof = ctx.canvas_dof(mb.copy(), inp["depth"], **dict(shs_gpu.Context.FX_DEFAULTS["dof"], **p["dof"]))[0]
    assert np.array_equal(dof, XR.ref_dof(mb, inp["depth"], **p["dof"]))
    bloom = ctx.canvas_spec_bright(inp["spec"], **p["spec_bright"])
    assert np.array_equal(bloom, XR.ref_spec_bright(inp["spec"], **p["spec_bright"]))
    for _ in range(10):
        bloom = ctx.canvas_gaussian_blur(ctx.canvas_gaussian_blur(bloom, True), False)
    st = XR.ref_glow_frame(inp, stages=True)
    assert np.array_equal(bloom, st["bloom"]), "bloom"
    flare, flare_pq = ctx.canvas_lens_flare(bloom, prequant=True, **p["lens_flare"])
    FX._check_pq(flare, flare_pq, XR.ref_lens_flare(bloom, **p["lens_flare"]), "whole frame: flare")
    final = ctx.canvas_additive(ctx.canvas_additive(dof, bloom), flare)
    assert np.array_equal(final, XR.ref_additive(XR.ref_additive(dof, bloom), flare))
    frame_out = dst.cpu().numpy()
    assert np.array_equal(frame_out, final), "the chain over the device planes differs from its passes one by one"
    assert (bloom[..., :3] > 0).any() and not np.array_equal(frame_out, got["color"])
