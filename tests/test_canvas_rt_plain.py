"""The camera passes of hello_per_object_motion_blur.cpp, hello_depth_of_field.cpp and hello_ping_pong.cpp on the GPU
(shs_rt_render_plain, shs_rt_frame::shading 8, 9 and 10), the first demo's blur (shs_canvas_object_blur) and the third's
Gaussian rounds (shs_canvas_ping_pong_blur) against tests/canvas_rt_plain_ref (test_canvas_rt_plain_ref.py holds the
wrapper, the scenes, the numpy witnesses and what pins the reference on the CPU).

Per frame, on every pixel of every plane, none excused (test_canvas_rt_skybox_ibl.compare_planes): the shading triangle,
the depth and the velocity equal bit for bit (every NaN one NaN, Inf as Inf); the pre-truncation colour floats within
helpers.TOL * 255, a NaN where the reference has a NaN; colour bytes equal but for a byte off by one where those floats
agree within that bound (helpers.assert_color_parity); the fourth prequant float, 1, bitwise.  The depth plane is compared
as it lies: in screen rows on both sides.

The blur is exact float arithmetic (no contraction, correctly rounded divide and sqrt, the x86-64 conversions): its bytes
are the restatement's on host and on device buffers.  The three whole-frame tests enqueue the raster and the demo's post
pass without a resolve in between and compare each stage with its restatement, the post pass's over the device's own raster
output, so that a byte the parity rule allows does not travel."""
import ctypes
import dataclasses

import numpy as np
import pytest

import helpers
import test_canvas_rt_motion_ref as M
import test_canvas_rt_plain_ref as PL
import test_canvas_rt_ref as R
import test_canvas_rt_sky as TK
from test_canvas_rt_plain_ref import H, W
from test_canvas_rt_skybox_ibl import _bits, compare_planes

pytestmark = pytest.mark.gpu
_P = ctypes.c_void_p


@pytest.fixture(scope="module")
def ctx():
    import shs_gpu
    c = shs_gpu.Context(0)
    yield c
    c.close()


def check_scene(c, name):
    frame, draws = PL.scene(name)
    ref = PL.scene_ref(name)
    c.rt_render_plain(frame, draws)
    got = TK._planes(c)
    compare_planes(got, ref, name)
    assert c.rt_stats() == ref["counters"]
    return got, ref


@pytest.mark.parametrize("name", list(PL.SCENES))
def test_scene(ctx, name):
    got, ref = check_scene(ctx, name)
    frame, _ = PL.scene(name)
    for call in (ctx.rt_resolve_spec, ctx.rt_device_spec):            # no spec plane after a plain pass
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == -1
    shown = got["tri_id"] >= 0
    assert (got["prequant"][..., 3][shown] == 1).all()
    assert (got["depth"][::-1][~shown].view(np.uint32) == np.float32(helpers.FLT_MAX).view(np.uint32)).all()
    assert (got["color"][~shown] == np.array(frame.clear_color, np.uint8)).all() and not got["velocity"][~shown].any()
    if frame.shading != 8:
        assert not got["velocity"].any()


def test_rejections_leave_the_previous_frame_unchanged():
    import shs_gpu
    frame, draws = PL.scene("windings")
    ref = PL.scene_ref("windings")
    with shs_gpu.Context(0) as c:
        def rejected(call, what):
            with pytest.raises(shs_gpu.ShsError) as e:
                call()
            assert e.value.code == -1, what

        c.rt_render_plain(frame, draws)
        compare_planes(TK._planes(c), ref, "before the rejections")
        rep = dataclasses.replace
        cases = [(f"shading {s}", lambda s=s: c.rt_render_plain(rep(frame, shading=s), draws)) for s in (0, 1, 2, 3, 4, 5, 6, 7, 11, -1)]
        for s in (8, 9, 10):
            f = rep(frame, shading=s)
            cases += [(f"shading {s} through shs_rt_render", lambda f=f: c.rt_render(f, draws)),
                      (f"shading {s} through shs_rt_render_motion", lambda f=f: c.rt_render_motion(f, draws)),
                      (f"shading {s} through shs_rt_render_pbr", lambda f=f: c.rt_render_pbr(f, draws, [shs_gpu.RtPbrDraw() for _ in draws])),
                      (f"shading {s} through shs_rt_render_pbr_soft", lambda f=f: c.rt_render_pbr_soft(f, draws, [shs_gpu.RtPbrDraw() for _ in draws])),
                      (f"shading {s} through shs_rt_render_skybox_ibl",
                       lambda f=f: c.rt_render_skybox_ibl(f, draws, [shs_gpu.RtSkyboxIblDraw() for _ in draws])),
                      (f"shading {s} through shs_rt_render_water",
                       lambda f=f: c.rt_render_water(f, draws, [shs_gpu.RtWaterDraw() for _ in draws], shs_gpu.RtWater()))]
        cases += [("width 0", lambda: c.rt_render_plain(rep(frame, width=0), draws)),
                  ("height -3", lambda: c.rt_render_plain(rep(frame, height=-3), draws)),
                  ("tile 0", lambda: c.rt_render_plain(rep(frame, ref_tile=(0, 80)), draws)),
                  ("tile -1", lambda: c.rt_render_plain(rep(frame, ref_tile=(80, -1)), draws)),
                  ("SHS_RT_USE_SHADOW", lambda: c.rt_render_plain(rep(frame, use_shadow=True), draws)),
                  ("SHS_RT_PCF", lambda: c.rt_render_plain(rep(frame, pcf=True), draws)),
                  ("albedo_tex", lambda: c.rt_render_plain(frame, [rep(draws[0], albedo_tex=R.TEX)] + draws[1:])),
                  ("unknown mesh", lambda: c.rt_render_plain(frame, [rep(draws[0], mesh=999)] + draws[1:]))]
        for what, call in cases:
            rejected(call, what)
            compare_planes(TK._planes(c), ref, f"after the rejection of {what}")
        # unknown flag bits, which the Python frame cannot spell
        fc = c._rt_frame_c(frame)
        fc.flags |= 64
        assert c._lib.shs_rt_render_plain(c._h, ctypes.byref(fc), c._rt_draw_array(draws), len(draws)) == -1
        compare_planes(TK._planes(c), ref, "after the rejection of unknown flags")
        # max_velocity_px is not read: what shs_rt_render_motion rejects is accepted here and changes nothing
        c.rt_render_plain(rep(frame, max_velocity_px=float("nan")), draws)
        compare_planes(TK._planes(c), ref, "with a NaN max_velocity_px")

        # a shading-6 frame's planes, and its spec rule, survive the rejections too
        f6, d6 = M.scene("windings")
        r6 = M.scene_ref("windings")
        c.rt_render_motion(f6, d6)
        for what, call in cases[:10] + cases[-8:]:
            rejected(call, what)
            compare_planes(TK._planes(c), r6, f"a shading-6 frame after the rejection of {what}")
            rejected(c.rt_resolve_spec, "spec after a shading-6 frame")
        # and a star frame's spec plane is still served after a rejected plain frame, and gone after an accepted one
        star, sdraws = M.scene("demo7")
        c.rt_render_motion(star, sdraws)
        spec = c.rt_resolve_spec()
        rejected(lambda: c.rt_render_plain(rep(frame, shading=7), draws), "shading 7")
        assert np.array_equal(_bits(c.rt_resolve_spec()), _bits(spec))
        c.rt_render_plain(frame, draws)
        rejected(c.rt_resolve_spec, "spec after a plain frame")
        rejected(c.rt_device_spec, "device spec after a plain frame")


def test_shading_0_is_undisturbed_by_plain_frames(ctx):
    """A shading-0 frame before and after plain frames of the three shadings on the same context: bit-identical planes."""
    view, lvp, draws = R.scene_demo()
    ctx.rt_render_shadow(R.SM, lvp, draws)
    ctx.rt_render(R._frame(view, lvp), draws)
    before = TK._planes(ctx)
    stats = ctx.rt_stats()
    for name in ("demo8", "demo9", "demo10", "odd16_8"):
        frame, pdraws = PL.scene(name)
        ctx.rt_render_plain(frame, pdraws)
    ctx.rt_render(R._frame(view, lvp), draws)
    after = TK._planes(ctx)
    for k in before:
        assert np.array_equal(after[k].view(np.uint8), before[k].view(np.uint8)), f"plane {k} differs"
    assert ctx.rt_stats() == stats and (before["tri_id"] >= 0).sum() > 3000


def test_sky_background_follows_the_plain_pass(ctx):
    """With a sky bound the background pass colours the pixels the raster left without a fragment, as after every camera
    pass; depth (in screen rows), velocity and ids stay the raster's."""
    import test_canvas_rt_skybox_ibl_ref as I
    frame, draws = PL.scene("demo8")
    ref = PL.scene_ref("demo8")
    ctx.rt_set_sky(I.demo_sky("analytic"))
    try:
        ctx.rt_render_plain(frame, draws)
        got = TK._planes(ctx)
    finally:
        ctx.rt_set_sky(None)
    shown = ref["tri_id"] >= 0
    assert np.array_equal(got["tri_id"], ref["tri_id"]) and np.array_equal(_bits(got["depth"]), _bits(ref["depth"]))
    assert np.array_equal(_bits(got["velocity"]), _bits(ref["velocity"]))
    helpers.assert_color_parity(got["color"][shown][None], ref["color"][shown][None], got["prequant"][shown][None], ref["prequant"][shown][None])
    assert (got["color"][~shown] != np.array(frame.clear_color, np.uint8)).any(-1).mean() > 0.99


# ---- shs_canvas_object_blur -----------------------------------------------------------------------------------------

BLUR_SETS = {"demo": {}, "canvas_rows": dict(depth_rows=0), "fast_64": dict(velocity_scale=4.0, max_samples=64),
             "slow_2": dict(velocity_scale=0.25, max_samples=2), "no_threshold": dict(multiplier=1.0, min_vel2=0.0, depth_eps=0.0)}


@pytest.mark.parametrize("name", list(BLUR_SETS))
def test_object_blur_is_the_restatements_bytes(ctx, name):
    import torch
    inp = PL.blur_inputs()
    over = BLUR_SETS[name]
    ref, gathered = PL.ref_object_blur(inp["src"], inp["depth"], inp["vel"], **over)
    assert gathered > 500
    got = ctx.canvas_object_blur(inp["src"], inp["depth"], inp["vel"], **over)
    assert np.array_equal(got, ref), f"host buffers: {int((got != ref).any(-1).sum())} pixels differ"
    dev = [torch.from_numpy(np.array(inp[k])).cuda() for k in ("src", "depth", "vel")]
    out = ctx.canvas_object_blur(*dev, **over)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref), "device buffers"


def test_object_blur_sizes_and_rejections(ctx):
    """One pixel, one row, one column, one past a block in both axes; then what the entry refuses."""
    import shs_gpu
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (7, 1), (1, 7), (65, 5)):
        src = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        depth = rng.choice(np.array([3.0, 3.1, 9.0, helpers.FLT_MAX], np.float32), (h, w))
        vel = rng.normal(0.0, 5.0, (h, w, 2)).astype(np.float32)
        for rows in (0, 1):
            got = ctx.canvas_object_blur(src, depth, vel, depth_rows=rows)
            assert np.array_equal(got, PL.ref_object_blur(src, depth, vel, depth_rows=rows)[0]), (w, h, rows)
    inp = PL.blur_inputs()
    for over in (dict(max_samples=1), dict(max_samples=65), dict(depth_rows=2), dict(depth_rows=-1), dict(multiplier=float("nan")),
                 dict(velocity_scale=float("inf")), dict(min_vel2=float("nan")), dict(depth_eps=float("nan"))):
        with pytest.raises(shs_gpu.ShsError) as e:
            ctx.canvas_object_blur(inp["src"], inp["depth"], inp["vel"], **over)
        assert e.value.code == -1, over
    src = np.array(inp["src"])
    d = ctx.fx_desc("object_blur", src.shape[1], src.shape[0])
    args = (ctypes.byref(d), _P(src.ctypes.data), _P(inp["depth"].ctypes.data), _P(inp["vel"].ctypes.data))
    assert ctx._lib.shs_canvas_object_blur(ctx._h, *args, _P(src.ctypes.data), 0) == -1           # dst overlaps src
    assert ctx._lib.shs_canvas_object_blur(ctx._h, *args, _P(src.ctypes.data + 4), 0) == -1
    assert ctx._lib.shs_canvas_object_blur(ctx._h, *args, _P(np.empty_like(src).ctypes.data), 2) == -1   # an unknown flag
    assert np.array_equal(src, inp["src"])


# ---- shs_canvas_ping_pong_blur --------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", [0, 1, 3])
def test_ping_pong_blur_is_the_gaussian_applied_twice_per_iteration(ctx, iterations):
    import shs_gpu
    import torch
    src = np.array(PL.blur_inputs()["src"])
    want = src
    for _ in range(iterations):
        want = ctx.canvas_gaussian_blur(ctx.canvas_gaussian_blur(want, True), False)
    got = ctx.canvas_ping_pong_blur(src.copy(), iterations)
    assert np.array_equal(got, want), "host buffers"
    dev = torch.from_numpy(src.copy()).cuda()
    ctx.canvas_ping_pong_blur(dev, iterations)
    ctx.synchronize()
    assert np.array_equal(dev.cpu().numpy(), want), "device buffers"
    assert (iterations == 0) == np.array_equal(want, src)
    with pytest.raises(shs_gpu.ShsError) as e:
        ctx.canvas_ping_pong_blur(src.copy(), -1)
    assert e.value.code == -1


# ---- the three whole frames -----------------------------------------------------------------------------------------

def test_per_object_blur_whole_frame_on_the_device(ctx):
    """hello_per_object_motion_blur.cpp's frame at 160 x 120: rt_render_plain (shading 8), then shs_canvas_object_blur with
    depth_rows 1 over rt_device_targets, nothing resolved in between."""
    import torch
    frame, draws = PL.scene("demo8")
    ctx._on_torch_stream()
    ctx.rt_render_plain(frame, draws)
    c_dev, d_dev, v_dev = ctx.rt_device_targets()
    dst = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    d = ctx.fx_desc("object_blur", W, H)
    assert d.depth_rows == 1
    ctx._check(ctx._lib.shs_canvas_object_blur(ctx._h, ctypes.byref(d), _P(c_dev), _P(d_dev), _P(v_dev), _P(dst.data_ptr()), ctx.CANVAS_DEVICE))
    ctx.synchronize()
    got = TK._planes(ctx)
    compare_planes(got, PL.scene_ref("demo8"), "whole frame: the raster (shading 8)")
    want, gathered = PL.ref_object_blur(got["color"], got["depth"], got["velocity"])
    out = dst.cpu().numpy()
    assert np.array_equal(out, want), f"{int((out != want).any(-1).sum())} pixels differ from the restatement over the device's planes"
    assert gathered > 500 and (out != got["color"]).any(-1).sum() > 200
    # the orientation matters on this scene: the same blur told the plane is in canvas rows gives another image
    assert not np.array_equal(want, PL.ref_object_blur(got["color"], got["depth"], got["velocity"], depth_rows=0)[0])


def test_depth_of_field_whole_frame_on_the_device(ctx):
    """hello_depth_of_field.cpp's frame at 160 x 120: rt_render_plain (shading 9), then shs_canvas_dof over
    rt_device_targets -- the depth plane as it lies, in screen rows, which is what that demo's autofocus and composite index
    -- nothing resolved in between; the focus depth comes back with the call."""
    from oracle import oracle
    frame, draws = PL.scene("demo9")
    ctx._on_torch_stream()
    ctx.rt_render_plain(frame, draws)
    c_dev, d_dev, _ = ctx.rt_device_targets()
    kw = dict(iterations=3, radius=6, focus=None, range_=24.0, max_blur=0.6)     # hello_depth_of_field.cpp's constants
    d = ctx.fx_desc("dof", W, H, kw)
    focus = ctypes.c_float()
    ctx._check(ctx._lib.shs_canvas_dof(ctx._h, ctypes.byref(d), _P(c_dev), _P(d_dev), None, ctypes.byref(focus), ctx.CANVAS_DEVICE))
    final, depth, _ = ctx.rt_resolve()                                           # (the colour plane was composited in place)
    ref = PL.scene_ref("demo9")
    assert np.array_equal(ctx.rt_resolve_ids(), ref["tri_id"]) and np.array_equal(_bits(depth), _bits(ref["depth"]))
    # the raster's own colour, from a second frame on the same context
    ctx.rt_render_plain(frame, draws)
    got = TK._planes(ctx)
    compare_planes(got, ref, "whole frame: the raster (shading 9)")
    want, _, want_focus = oracle.canvas_dof(got["color"], got["depth"], **kw)
    assert np.array_equal(final, want), f"{int((final != want).any(-1).sum())} pixels differ from the restatement over the device's planes"
    assert focus.value == want_focus and focus.value != 15.0
    assert (final != got["color"]).any(-1).sum() > 200
    # the demo's flipped read shows: over the plane turned the right way up the composite is another image
    assert not np.array_equal(want, oracle.canvas_dof(got["color"], got["depth"][::-1], **kw)[0])


def test_ping_pong_whole_frame_on_the_device(ctx):
    """hello_ping_pong.cpp's frame at 160 x 120: rt_render_plain (shading 10), then shs_canvas_ping_pong_blur with three
    iterations on the colour plane in place, nothing resolved in between."""
    from oracle import oracle
    frame, draws = PL.scene("demo10")
    ctx._on_torch_stream()
    ctx.rt_render_plain(frame, draws)
    c_dev, _, _ = ctx.rt_device_targets()
    ctx._check(ctx._lib.shs_canvas_ping_pong_blur(ctx._h, W, H, 3, _P(c_dev), ctx.CANVAS_DEVICE))
    final, depth, vel = ctx.rt_resolve()
    ref = PL.scene_ref("demo10")
    assert np.array_equal(_bits(depth), _bits(ref["depth"])) and not vel.any()
    ctx.rt_render_plain(frame, draws)
    got = TK._planes(ctx)
    compare_planes(got, ref, "whole frame: the raster (shading 10)")
    want = got["color"]
    for _ in range(3):
        want = oracle.canvas_gaussian(oracle.canvas_gaussian(want, True), False)
    assert np.array_equal(final, want), f"{int((final != want).any(-1).sum())} pixels differ from the restatement over the device's planes"
    assert (final != got["color"]).any(-1).sum() > 200
